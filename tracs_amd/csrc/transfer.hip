// transfer.hip -- transfer bootstrap support for the neighbour-joining tree (tracs_transfer_*, include/tracs_hip.h).
//
// For an internal edge e of the main tree (S_e = the leaves below its child, s = |S_e|) and every edge f of a replicate tree (T_f below
// its child, t = |T_f|): h = s + t - 2 |S_e & T_f|, delta = min(h, n - h), phi(e) = the smallest delta over all 2n - 3 edges f.  The
// sums of phi over the replicates and p_e = min(s, n - s) are what the host turns into the support 1 - Phi / (B (p - 1)).
//
// No (main edge, replicate node) count array exists anywhere.  The host turns a replicate into a post-order PROGRAM of 2n - 3 entries
// (a leaf: its id; a joined node: 0x80000000 | its subtree's size, after its two subtrees; the top node: nothing), children visited
// largest subtree first, so that "leaf: push; joined node: pop two, push the sum" never holds more than floor(log2 n) + 3 values.  On
// the device one lane owns one main edge and runs that program on a stack of |S_e & T_f| counts:
//     membership   Mt[leaf][ceil((n - 3) / 64)] 64-bit words: bit k of word w of row l = leaf l is in S_e of the (64 w + k)-th internal
//                  edge of the main tree in creation order.  Built once per main tree, on the host, from tree_bitsets' bitsets.
//     transfer_phi_kernel   one wave per 64 main edges.  The program entry, the subtree size, the stack depth and the address of the
//                  one Mt word the wave needs for a leaf are wave-uniform; only the counts are per lane.
#include "common.h"
#include "pair_select.h"
#include "debug_api.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>

namespace tracs {

namespace {

constexpr size_t TR_MAX_LEAVES = 1u << 24;      // as the neighbour-joining state: node ids and sizes stay far inside 31 bits
constexpr unsigned TR_STACK = 40;               // the kernel's stack: floor(log2 2^24) + 3 = 27 values at most
constexpr unsigned TR_INTERNAL = 0x80000000u;

struct Hdr {
    unsigned long long n;            // leaves the state was initialised for
};

struct State {
    Hdr *hdr;
    unsigned long long *Mt;          // [n][W]
    unsigned long long *sum;         // per internal edge of the main tree, in creation order: the sum of phi
    unsigned *size, *edge;           // ... |S_e| and the edge's index among the 2n - 3
    unsigned *program;               // the replicate being added
    size_t nI, W;
    State(void *base, size_t n, size_t *bytes = nullptr)
    {
        nI = n > 3 ? n - 3 : 0;
        W = (nI + 63) / 64;
        const size_t cap = std::max<size_t>(n, 4);
        Arena a(base, bytes);
        hdr = reinterpret_cast<Hdr *>(a.take<char>(256));
        Mt = a.take<unsigned long long>(cap * std::max<size_t>(W, 1));
        sum = a.take<unsigned long long>(cap);
        size = a.take<unsigned>(cap); edge = a.take<unsigned>(cap);
        program = a.take<unsigned>(2 * cap);
    }
};

__device__ __forceinline__ unsigned readlane32(unsigned v, unsigned k) { return (unsigned)__builtin_amdgcn_readlane((int)v, (int)k); }

// One lane = one internal edge of the main tree, one wave (= one workgroup) = 64 of them; every lane stays active to the end, so that
// readlane never reads a lane that did not load (lanes past the last edge run with s = 0 against all-zero Mt bits and store nothing).
// The program comes in windows of 64 entries: lane i loads entry i of the window with one coalesced load and, where it is a leaf, the
// wave's word of that leaf's Mt row, so global latency is paid once per 64 steps; the loads run two windows (entries) and one window
// (words) ahead of the steps.  The steps take entry and word out with v_readlane, which makes them scalar: the branch on the entry's
// kind, the stack depth and the LDS address are uniform.  The stack is LDS [depth][lane] (a lane only ever touches its own column: no
// barrier) with the top value in a register.  A step: leaf -- push the lane's bit; joined node -- pop two, push the sum c; then
// h = s + t - 2 c, min(h, n - h), min into phi.  (c <= min(s, t) and s + t - c <= n, so 0 <= h <= n in unsigned arithmetic.)
__global__ __launch_bounds__(64) void transfer_phi_kernel(State st, unsigned n, unsigned len, unsigned *__restrict__ phi_out)
{
    __shared__ unsigned stack[TR_STACK * 64];
    const unsigned lane = threadIdx.x;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x);
    const unsigned k = wave * 64 + lane;
    const bool mine = k < st.nI;
    const unsigned s = mine ? st.size[k] : 0u;
    const unsigned long long *__restrict__ mt = st.Mt + wave;
    const unsigned *__restrict__ prog = st.program;
    const size_t W = st.W;
    auto entry_at = [&](unsigned at) { return at < len ? prog[at] : TR_INTERNAL; };
    auto word_of = [&](unsigned e) { return (e & TR_INTERNAL) ? 0ull : mt[(size_t)e * W]; };

    unsigned e0 = entry_at(lane), e1 = entry_at(64 + lane);
    unsigned long long w0 = word_of(e0);
    unsigned phi = 0xFFFFFFFFu, top = 0, sp = 0;                         // sp values on the stack: sp - 1 of them in LDS, the last in `top`
    for (unsigned at = 0; at < len; at += 64) {
        const unsigned e2 = entry_at(at + 128 + lane);
        const unsigned long long w1 = word_of(e1);
        const unsigned cnt = min(64u, len - at);
        for (unsigned i = 0; i < cnt; i++) {
            const unsigned iu = __builtin_amdgcn_readfirstlane(i);
            const unsigned e = readlane32(e0, iu);
            unsigned t;
            if (e & TR_INTERNAL) {                                       // (uniform) pop two, push their sum
                t = e & ~TR_INTERNAL;
                top += stack[(sp - 2) * 64 + lane];
                sp -= 1;
            } else {
                const unsigned lo = readlane32((unsigned)w0, iu), hi = readlane32((unsigned)(w0 >> 32), iu);
                if (sp) stack[(sp - 1) * 64 + lane] = top;
                top = ((lane < 32 ? lo : hi) >> (lane & 31u)) & 1u;
                sp += 1;
                t = 1;
            }
            const unsigned h = s + t - 2u * top;
            phi = min(phi, min(h, n - h));
        }
        e0 = e1; w0 = w1; e1 = e2;
    }
    if (mine) {
        st.sum[k] += (unsigned long long)phi;
        if (phi_out) phi_out[st.edge[k]] = phi;
    }
}

// the strict form of tree_bitsets' check: every joined node has two children and the top node three (what tracs_nj_edges gives)
int binary_tree_check(const char *who, size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges, std::vector<uint64_t> *below)
{
    std::vector<uint32_t> kids;
    int rc;
    if ((rc = tree_bitsets(who, n, parent, child, n_edges, below, &kids))) return rc;
    const uint32_t top = parent[n_edges - 1];
    for (size_t v = n; v < 2 * n - 2; v++)
        if (kids[v] != (v == top ? 3u : 2u)) { set_error(std::string(who) + ": the edges are not a tree in creation order"); return TRACS_E_ARG; }
    return TRACS_OK;
}

}  // namespace

int transfer_add_program(void *state, size_t n, const uint32_t *program, size_t depth, uint32_t *phi, hipStream_t stream)
{
    if (n < 4) return TRACS_OK;
    if (!state || !program) { set_error("tracs_transfer_add: NULL argument"); return TRACS_E_ARG; }
    if (depth > TR_STACK) {
        set_error("tracs_transfer_add: the program needs a stack of " + std::to_string(depth) + " values, the kernel has " + std::to_string(TR_STACK));
        return TRACS_E_ARG;
    }
    DeviceCall guard(stream);
    State s(state, n);
    Hdr h{};
    int rc;
    if ((rc = read_state_header(s.hdr, n, "tracs_transfer_add", stream, &h))) return rc;
    const unsigned len = (unsigned)(2 * n - 3);
    TRACS_HIP_CHECK(hipMemcpyAsync(s.program, program, (size_t)len * 4, hipMemcpyHostToDevice, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));                        // (the program is the caller's memory; the kernel is stream-ordered)
    hipLaunchKernelGGL(transfer_phi_kernel, dim3((unsigned)s.W), dim3(64), 0, stream, s, (unsigned)n, len, phi);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

}  // namespace tracs

using namespace tracs;

extern "C" {

// Host only, no recursion.  Children largest subtree first (ties: lower id); a node is emitted when its last child is complete.
int tracs_tree_transfer_program(size_t n, const uint32_t *rep_parent, const uint32_t *rep_child, size_t n_edges, uint32_t *program, size_t *depth)
{
    if (depth) *depth = 0;
    if (n < 4) return TRACS_OK;                                           // no internal edge: nothing to compare with
    if (!rep_parent || !rep_child || !program || !depth) { set_error("tracs_tree_transfer_program: NULL argument"); return TRACS_E_ARG; }
    if (n > TR_MAX_LEAVES) { set_error("tracs_tree_transfer_program: more than 2^24 leaves"); return TRACS_E_ARG; }
    int rc;
    if ((rc = binary_tree_check("tracs_tree_transfer_program", n, rep_parent, rep_child, n_edges, nullptr))) return rc;
    const size_t n_nodes = 2 * n - 2;
    const uint32_t top = rep_parent[n_edges - 1];
    std::vector<uint32_t> size(n_nodes, 0), kid(3 * (n_nodes - n), 0), have(n_nodes - n, 0);
    for (size_t v = 0; v < n; v++) size[v] = 1;
    for (size_t e = 0; e < n_edges; e++) {                                // (a child is complete before the edge that hangs it)
        const uint32_t p = rep_parent[e], c = rep_child[e];
        size[p] += size[c];
        kid[3 * (p - n) + have[p - n]++] = c;
    }
    for (size_t v = n; v < n_nodes; v++) {
        uint32_t *k = &kid[3 * (v - n)];
        std::sort(k, k + have[v - n], [&](uint32_t a, uint32_t b) { return size[a] != size[b] ? size[a] > size[b] : a < b; });
    }
    struct Frame { uint32_t node, next; };
    std::vector<Frame> stack;
    stack.push_back({top, 0});
    size_t at = 0, sp = 0, deepest = 0;
    while (!stack.empty()) {
        Frame &f = stack.back();
        if (f.next == have[f.node - n]) {
            const uint32_t node = f.node;
            stack.pop_back();
            if (node != top) { program[at++] = 0x80000000u | size[node]; sp -= 1; }
            continue;
        }
        const uint32_t c = kid[3 * (f.node - n) + f.next++];
        if (c < n) { program[at++] = c; sp += 1; deepest = std::max(deepest, sp); }
        else stack.push_back({c, 0});
    }
    if (at != n_edges || sp != 3) { set_error("tracs_tree_transfer_program: the edges are not a tree in creation order"); return TRACS_E_ARG; }
    *depth = deepest;
    return TRACS_OK;
}

size_t tracs_transfer_state_bytes(size_t n)
{
    if (n > TR_MAX_LEAVES) return 0;
    return arena_bytes<State>(n);
}

// The membership matrix and the sizes on the host, one upload each; the sums zeroed.  seconds (measurement, may be NULL): the host's
// share (bitsets + transposition) and the uploads with the stream drained.
static int transfer_init(void *state, size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges, hipStream_t stream, double *seconds)
{
    if (!state) { set_error("tracs_transfer_init: NULL state"); return TRACS_E_ARG; }
    if (!tracs_transfer_state_bytes(n)) { set_error("tracs_transfer_init: more than 2^24 leaves"); return TRACS_E_ARG; }
    const auto t0 = std::chrono::steady_clock::now();
    DeviceCall guard(stream);
    State s(state, n);
    Hdr h{};
    h.n = n;
    if (n < 4) {
        TRACS_HIP_CHECK(hipMemcpyAsync(s.hdr, &h, sizeof h, hipMemcpyHostToDevice, stream));
        TRACS_HIP_CHECK(hipStreamSynchronize(stream));
        return TRACS_OK;
    }
    if (!parent || !child) { set_error("tracs_transfer_init: NULL argument"); return TRACS_E_ARG; }
    std::vector<uint64_t> below;
    int rc;
    if ((rc = binary_tree_check("tracs_transfer_init", n, parent, child, n_edges, &below))) return rc;
    const size_t Wn = (n + 63) / 64, W = s.W;
    std::vector<uint64_t> Mt(n * W, 0);
    std::vector<uint32_t> size(s.nI), edge(s.nI);
    size_t k = 0;
    for (size_t e = 0; e < n_edges; e++) {
        if (child[e] < n) continue;
        const uint64_t *row = &below[(child[e] - n) * Wn];
        const uint64_t bit = 1ull << (k & 63);
        uint32_t count = 0;
        for (size_t w = 0; w < Wn; w++)
            for (uint64_t x = row[w]; x; x &= x - 1) {
                Mt[(w * 64 + (size_t)__builtin_ctzll(x)) * W + (k >> 6)] |= bit;
                count++;
            }
        size[k] = count;
        edge[k] = (uint32_t)e;
        k++;
    }
    if (k != s.nI) { set_error("tracs_transfer_init: the edges are not a tree in creation order"); return TRACS_E_ARG; }
    const auto t1 = std::chrono::steady_clock::now();
    TRACS_HIP_CHECK(hipMemcpyAsync(s.Mt, Mt.data(), Mt.size() * 8, hipMemcpyHostToDevice, stream));
    TRACS_HIP_CHECK(hipMemcpyAsync(s.size, size.data(), s.nI * 4, hipMemcpyHostToDevice, stream));
    TRACS_HIP_CHECK(hipMemcpyAsync(s.edge, edge.data(), s.nI * 4, hipMemcpyHostToDevice, stream));
    TRACS_HIP_CHECK(hipMemsetAsync(s.sum, 0, s.nI * 8, stream));
    TRACS_HIP_CHECK(hipMemcpyAsync(s.hdr, &h, sizeof h, hipMemcpyHostToDevice, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));                        // (the uploads read this frame's vectors)
    if (seconds) {
        seconds[0] = std::chrono::duration<double>(t1 - t0).count();
        seconds[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    }
    return TRACS_OK;
}

int tracs_transfer_init(void *state, size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges, void *stream)
{
    return transfer_init(state, n, parent, child, n_edges, static_cast<hipStream_t>(stream), nullptr);
}

int tracs_transfer_add(void *state, size_t n, const uint32_t *rep_parent, const uint32_t *rep_child, size_t rep_n_edges, uint32_t *phi, void *stream)
{
    if (n < 4) return TRACS_OK;
    if (!state) { set_error("tracs_transfer_add: NULL state"); return TRACS_E_ARG; }
    if (n > TR_MAX_LEAVES) { set_error("tracs_transfer_add: more than 2^24 leaves"); return TRACS_E_ARG; }
    std::vector<uint32_t> program(2 * n - 3);
    size_t depth = 0;
    int rc;
    if ((rc = tracs_tree_transfer_program(n, rep_parent, rep_child, rep_n_edges, program.data(), &depth))) return rc;
    return transfer_add_program(state, n, program.data(), depth, phi, static_cast<hipStream_t>(stream));
}

int tracs_transfer_emit(void *state, size_t n, uint64_t *sum_phi, uint32_t *light)
{
    if (!state) { set_error("tracs_transfer_emit: NULL state"); return TRACS_E_ARG; }
    if (n > TR_MAX_LEAVES) { set_error("tracs_transfer_emit: more than 2^24 leaves"); return TRACS_E_ARG; }
    hipStream_t stream = nullptr;                                         // (a call on another stream before this one: DeviceCall drains the device)
    DeviceCall guard(stream);
    State s(state, n);
    Hdr h{};
    int rc;
    if ((rc = read_state_header(s.hdr, n, "tracs_transfer_emit", stream, &h))) return rc;
    if (n < 4) return TRACS_OK;
    std::vector<uint64_t> sum(s.nI);
    std::vector<uint32_t> size(s.nI), edge(s.nI);
    TRACS_HIP_CHECK(hipMemcpyAsync(sum.data(), s.sum, s.nI * 8, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipMemcpyAsync(size.data(), s.size, s.nI * 4, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipMemcpyAsync(edge.data(), s.edge, s.nI * 4, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    for (size_t k = 0; k < s.nI; k++) {
        if (edge[k] >= 2 * n - 3) { set_error("tracs_transfer_emit: the state holds no main tree"); return TRACS_E_ARG; }
        if (sum_phi) sum_phi[edge[k]] = sum[k];
        if (light) light[edge[k]] = std::min<uint32_t>(size[k], (uint32_t)n - size[k]);
    }
    return TRACS_OK;
}

// The one-shot sibling of tracs_tree_support: host arrays; a state of its own; phi (uint32 per edge of the first tree) <- phi of its
// internal edges against the second tree, other entries left alone.
int tracs_tree_transfer(size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges, const uint32_t *rep_parent,
                        const uint32_t *rep_child, size_t rep_n_edges, uint32_t *phi)
{
    if (n < 4) return TRACS_OK;
    if (!parent || !child || !rep_parent || !rep_child || !phi) { set_error("tracs_tree_transfer: NULL argument"); return TRACS_E_ARG; }
    const size_t bytes = tracs_transfer_state_bytes(n);
    if (!bytes) { set_error("tracs_tree_transfer: more than 2^24 leaves"); return TRACS_E_ARG; }
    if (n_edges != 2 * n - 3) { set_error("tracs_tree_transfer: a tree over n leaves has 2n - 3 edges"); return TRACS_E_ARG; }
    DeviceArray<char> buf;
    int rc = buf.alloc(bytes + n_edges * 4, "transfer state and phi");
    if (rc) return rc;
    char *const d = buf.get();
    uint32_t *d_phi = reinterpret_cast<uint32_t *>(d + bytes);
    std::vector<uint32_t> got(n_edges);
    if ((rc = tracs_transfer_init(d, n, parent, child, n_edges, nullptr)) ||
        (rc = tracs_transfer_add(d, n, rep_parent, rep_child, rep_n_edges, d_phi, nullptr))) return rc;
    TRACS_HIP_CHECK(hipMemcpy(got.data(), d_phi, n_edges * 4, hipMemcpyDeviceToHost));
    for (size_t e = 0; e < n_edges; e++) if (child[e] >= n) phi[e] = got[e];
    return TRACS_OK;
}

// Measurement (scripts/bench_transfer.py): tracs_transfer_init with the host's share and the uploads timed apart -> seconds[2]
int tracs_debug_transfer_init(void *state, size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges, double *seconds)
{
    if (!seconds) { set_error("tracs_debug_transfer_init: NULL argument"); return TRACS_E_ARG; }
    seconds[0] = seconds[1] = 0.0;
    return transfer_init(state, n, parent, child, n_edges, nullptr, seconds);
}

}  // extern "C"
