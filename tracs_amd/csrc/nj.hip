// nj.hip -- neighbour joining on the dense distance matrix (tracs_nj_*, include/tracs_hip.h).
//
// Canonical neighbour joining (Saitou & Nei; Q as Studier & Keppler) in IEEE float64, every operation and its order fixed (the
// definition: DESIGN.md 3.17, restated in tests/nj_ref.py): no fused multiply-add (the library is built with -ffp-contract=off and
// nothing here calls fma), one rounding per operation.  Leaves are the nodes 0 .. n - 1, join number t makes the node n + t.
//
// State: the matrix D (n x n f64, full symmetric, leading dimension n), per slot its row sum R and the id of the node that lives in
// it, the join records, the scan's per-workgroup partial winners and two rows of scratch.  The r active nodes always occupy the
// slots 0 .. r - 1, so the scanned block is dense (r x r) whatever has been joined.  One join step is three stream-ordered launches:
//   scan     every pair of slots i < j: Q = (r - 2) D_ij - (R_i + R_j); the smallest (Q, lower id, higher id) per lane -> wave
//            (shuffles) -> workgroup (LDS) -> one partial per workgroup; the workgroup that finishes last (a counter; nobody waits
//            on it) reduces the partials, writes the join's record and the two winning slots
//   rows     per slot k: D_uk and the new R_k from the rows of a and b (rows: D is symmetric, so they are coalesced) into the scratch
//            row `urow`, the last slot's row into the scratch row `lrow`; R only -- no cell of D is written
//   commit   u's row and column go into the smaller of the two winning slots, the last active slot moves into the larger one; reads
//            the scratch rows only, and every cell of D it writes is written by exactly one thread
// so no launch reads a cell of D that the same launch writes.  The formulas are symmetric in a and b and the order is on node ids:
// the result depends on neither the slot layout nor the move.  The host knows r at every step: the whole loop is enqueued without
// a read-back.
//
// BIONJ (Gascuel 1997; tracs_bionj_*, DESIGN.md 3.23, restated in tests/bionj_ref.py) is the same loop with a second matrix V of
// variances (V = D at the start) and its running row sums RV: the scan, the record and the three-node end are neighbour joining's, and
// the reduction weights the rows of a and b with the lambda that minimises the variance of the new row.  Gascuel's sum over k of
// V_bk - V_ak is RV_b - RV_a (the diagonal is 0 and V is symmetric, so the cells of a and b cancel): no order-dependent reduction and
// no further kernel.  lambda, mu = 1 - lambda, the two lengths and the new node's two sums are computed ONCE per join, by the thread
// that writes the record, and travel in the header; the rows kernel writes the scratch rows of both matrices, the commit kernel both
// matrices.  mu is rounded, so the formulas are NOT symmetric in a and b: a is the lower id (hdr->sa), never the lower slot.
// A BIONJ state is a neighbour-joining state followed by V, RV and V's two scratch rows: every other entry point sees the prefix.
#include "common.h"
#include "pair_select.h"
#include "debug_api.h"

#include <charconv>
#include <cmath>
#include <cstring>

using namespace tracs;

namespace {

constexpr unsigned NJ_SCAN_BLOCKS = 2048;       // at most this many workgroups (and partial winners) per scan
constexpr size_t NJ_MAX_NODES = 1u << 24;       // leaves of one state: slots and node ids stay 32-bit, n * n * 8 a size_t

struct Hdr {
    unsigned long long n;           // nodes the state was initialised for
    unsigned long long zero_pair;   // per-site loading: the smallest i << 32 | j with nn = 0 (KEY_NONE: none)
    unsigned long long ran;         // tracs_nj_run has been enqueued on this state
    unsigned counter;               // workgroups of the running scan that have published their partial
    unsigned sa, sb;                // the winning slots of the last scan (sa holds the lower id)
    unsigned last_ids[3];           // the last three nodes, by id (n = 2: the two leaves)
    double last_d[3];               // D_xy, D_xz, D_yz (n = 2: D_01)
    // BIONJ, the running join: lambda, mu, l_a, l_b, (lambda mu) V_ab, and the sums R_u, RV_u of the new node
    double lam, mu, la, lb, lmv, ru, rvu;
};

struct State {
    Hdr *hdr;
    double *D, *R, *urow, *lrow;
    unsigned *ids;
    unsigned *rec_a, *rec_b;
    double *rec_d, *rec_ra, *rec_rb;
    unsigned long long *pq, *pids, *pslots;
    double *V = nullptr, *RV = nullptr, *vurow = nullptr, *vlrow = nullptr;      // BIONJ only, after everything else
    State(void *base, size_t n, size_t *bytes = nullptr, bool bionj = false)
    {
        const size_t cap = std::max<size_t>(n, 1);
        Arena a(base, bytes);
        hdr = reinterpret_cast<Hdr *>(a.take<char>(256));
        D = a.take<double>(cap * cap);
        R = a.take<double>(cap); urow = a.take<double>(cap); lrow = a.take<double>(cap);
        ids = a.take<unsigned>(cap);
        rec_a = a.take<unsigned>(cap); rec_b = a.take<unsigned>(cap);
        rec_d = a.take<double>(cap); rec_ra = a.take<double>(cap); rec_rb = a.take<double>(cap);
        pq = a.take<unsigned long long>(NJ_SCAN_BLOCKS); pids = a.take<unsigned long long>(NJ_SCAN_BLOCKS);
        pslots = a.take<unsigned long long>(NJ_SCAN_BLOCKS);
        if (bionj) {
            V = a.take<double>(cap * cap);
            RV = a.take<double>(cap); vurow = a.take<double>(cap); vlrow = a.take<double>(cap);
        }
    }
};

// ---- loading ---------------------------------------------------------------------------------------------------------------------
// KIND 0: D_ij = d; 1: D_ij = d / nn (nn = 0: the pair is reported, the cell gets 0); 2: D_ij = src_ij (f64).  Cells j > i of the rows
// [r0, r1), indexed by ABSOLUTE row with leading dimension ld, mirrored into the column.  A state initialised for another n is left
// alone (tracs_nj_run reads the header and refuses it): loading stays asynchronous, one panel's load under the next panel's kernels.
template <int KIND>
__global__ __launch_bounds__(256) void nj_load_kernel(State s, size_t n, const void *__restrict__ src, const unsigned *__restrict__ ncomp,
                                                      size_t ld, size_t r0, size_t r1)
{
    if (s.hdr->n != n) return;
    for (size_t i = r0 + blockIdx.y; i < r1; i += gridDim.y)
        for (size_t j = i + 1 + (size_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (size_t)gridDim.x * 256) {
            double v;
            if (KIND == 2) v = static_cast<const double *>(src)[i * ld + j];
            else {
                v = (double)static_cast<const unsigned *>(src)[i * ld + j];
                if (KIND == 1) {
                    const unsigned nn = ncomp[i * ld + j];
                    if (nn == 0) { atomicMin(&s.hdr->zero_pair, ((unsigned long long)i << 32) | j); v = 0.0; }
                    else v = v / (double)nn;
                }
            }
            s.D[i * n + j] = v;
            s.D[j * n + i] = v;
        }
}

// R_k = the sum of D_mk over m = 0 .. n - 1 in that order, one add at a time (the diagonal's +0.0 included); slot k holds leaf k
__global__ __launch_bounds__(64) void nj_rowsum_kernel(State s, size_t n)
{
    const size_t k = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    double sum = 0.0;
    size_t m = 0;
    for (; m + 8 <= n; m += 8) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = s.D[(m + q) * n + k];
#pragma unroll
        for (int q = 0; q < 8; q++) sum = sum + v[q];
    }
    for (; m < n; m++) sum = sum + s.D[m * n + k];
    s.R[k] = sum;
    s.ids[k] = (unsigned)k;
}

// ---- the scan --------------------------------------------------------------------------------------------------------------------
// a candidate: Q, the pair's ids (lower << 32 | higher) and its slots (i << 32 | j).  No candidate: Q = +inf under KEY_NONE, with the
// slots (0, 1), so that even a matrix of NaNs leaves two valid slots behind.
struct Cand { double q; unsigned long long ids, slots; };

__device__ __forceinline__ Cand no_cand() { return Cand{__longlong_as_double(0x7FF0000000000000ll), KEY_NONE, 1ull}; }

__device__ __forceinline__ void offer(Cand &c, double q, unsigned long long ids, unsigned long long slots)
{
    if (q < c.q || (q == c.q && ids < c.ids)) { c.q = q; c.ids = ids; c.slots = slots; }
}

__device__ __forceinline__ Cand wave_best(Cand c)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const double q = __shfl_down(c.q, off, 64);
        const unsigned long long ids = __shfl_down(c.ids, off, 64), slots = __shfl_down(c.slots, off, 64);
        offer(c, q, ids, slots);
    }
    return c;
}

// the workgroup's best in thread 0 (every thread calls it)
__device__ __forceinline__ Cand block_best(Cand c, Cand *sh)
{
    c = wave_best(c);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; w++) offer(c, sh[w].q, sh[w].ids, sh[w].slots);
    return c;
}

// The active triangle is folded into a rectangle so that every workgroup step has the same amount to read: row f (its r - 1 - f
// cells j > f) is followed by row r - 2 - f (its f + 1 cells), r positions in all, for f < r / 2; the middle row of an even r stands
// alone.  A workgroup takes tiles of NJ_TILE positions of one folded row, eight cells per thread, the cells' loads ahead of their use;
// tiles are interleaved over the grid.  t: the join's number.
constexpr unsigned NJ_TILE = 2048;

// BIONJ: what one join needs besides its record, from the record's own values (a = the lower id, in slot sa), one rounding per
// operation, in the order tests/bionj_ref.py fixes.  The lengths are tracs_nj_edges's formula with the same operations.
__device__ __forceinline__ void bionj_scalars(const State &s, size_t n, unsigned r, unsigned sa, unsigned sb)
{
    Hdr *h = s.hdr;
    const double rm2 = (double)(r - 2), den = 2.0 * rm2;
    const double d = s.D[(size_t)sa * n + sb], v = s.V[(size_t)sa * n + sb];
    const double Ra = s.R[sa], Rb = s.R[sb], RVa = s.RV[sa], RVb = s.RV[sb];
    const double la = (0.5 * d) + ((Ra - Rb) / den);
    const double lb = d - la;
    double lam = 0.5;
    if (v != 0.0) {
        lam = 0.5 + ((RVb - RVa) / (den * v));
        if (lam < 0.0) lam = 0.0;
        if (lam > 1.0) lam = 1.0;
    }
    const double mu = 1.0 - lam;
    const double lmv = (lam * mu) * v;
    h->lam = lam; h->mu = mu; h->la = la; h->lb = lb; h->lmv = lmv;
    h->ru = (lam * ((Ra - d) - (rm2 * la))) + (mu * ((Rb - d) - (rm2 * lb)));
    h->rvu = ((lam * (RVa - v)) + (mu * (RVb - v))) - (rm2 * lmv);
}

template <bool BIONJ>
__global__ __launch_bounds__(256) void nj_scan_kernel(State s, size_t n, unsigned r, unsigned t)
{
    __shared__ Cand sh[4];
    __shared__ int is_last;
    const double rm2 = (double)(r - 2);
    const unsigned per_row = (r + NJ_TILE - 1) / NJ_TILE;
    const unsigned long long tiles = (unsigned long long)(r / 2) * per_row;
    Cand c = no_cand();
    for (unsigned long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const unsigned f = (unsigned)(tile / per_row), p0 = (unsigned)(tile % per_row) * NJ_TILE + threadIdx.x;
        const unsigned i1 = f, i2 = r - 2 - f, len1 = r - 1 - f, lim = i2 == i1 ? len1 : r;
        const double R1 = s.R[i1], R2 = s.R[i2];
        const unsigned id1 = s.ids[i1], id2 = s.ids[i2];
        const double *row1 = s.D + (size_t)i1 * n + (i1 + 1), *row2 = s.D + (size_t)i2 * n + (i2 + 1);
        double d[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const unsigned p = p0 + u * 256;
            d[u] = p < lim ? (p < len1 ? row1[p] : row2[p - len1]) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const unsigned p = p0 + u * 256;
            if (p < lim) {
                const bool first = p < len1;
                const unsigned i = first ? i1 : i2, j = first ? i1 + 1 + p : i2 + 1 + (p - len1);
                const double q = (rm2 * d[u]) - ((first ? R1 : R2) + s.R[j]);
                const unsigned idi = first ? id1 : id2, idj = s.ids[j];
                const unsigned lo = idi < idj ? idi : idj, hi = idi < idj ? idj : idi;
                offer(c, q, ((unsigned long long)lo << 32) | hi, ((unsigned long long)i << 32) | j);
            }
        }
    }
    c = block_best(c, sh);
    // publish the partial (write-through stores, then the release), count this workgroup; the last one to arrive reduces
    if (threadIdx.x == 0) {
        __hip_atomic_store(&s.pq[blockIdx.x], (unsigned long long)__double_as_longlong(c.q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s.pids[blockIdx.x], c.ids, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s.pslots[blockIdx.x], c.slots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        const unsigned before = __hip_atomic_fetch_add(&s.hdr->counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        is_last = before + 1 == gridDim.x;
    }
    __syncthreads();
    if (!is_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    c = no_cand();
    for (unsigned k = threadIdx.x; k < gridDim.x; k += 256) {
        const double q = __longlong_as_double((long long)__hip_atomic_load(&s.pq[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        offer(c, q, __hip_atomic_load(&s.pids[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
              __hip_atomic_load(&s.pslots[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    __syncthreads();                                    // (sh is reused)
    c = block_best(c, sh);
    if (threadIdx.x == 0) {
        unsigned sa = (unsigned)(c.slots >> 32), sb = (unsigned)(c.slots & 0xffffffffu);
        if (sa >= r || sb >= r || sa == sb) { sa = 0; sb = 1; }          // (cannot happen; the slots index memory)
        if (s.ids[sa] > s.ids[sb]) { const unsigned x = sa; sa = sb; sb = x; }
        s.hdr->sa = sa; s.hdr->sb = sb;
        s.rec_a[t] = s.ids[sa]; s.rec_b[t] = s.ids[sb];
        s.rec_d[t] = s.D[(size_t)sa * n + sb]; s.rec_ra[t] = s.R[sa]; s.rec_rb[t] = s.R[sb];
        if (BIONJ) bionj_scalars(s, n, r, sa, sb);
        __hip_atomic_store(&s.hdr->counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the update ------------------------------------------------------------------------------------------------------------------
// keep = the smaller winning slot (u's), ret = the larger (retired; the last slot r - 1 moves into it unless it is the last)
__global__ __launch_bounds__(256) void nj_rows_kernel(State s, size_t n, unsigned r, unsigned t)
{
    const unsigned k = blockIdx.x * 256 + threadIdx.x;
    if (k >= r) return;
    const unsigned sa = s.hdr->sa, sb = s.hdr->sb, keep = sa < sb ? sa : sb, ret = sa < sb ? sb : sa, last = r - 1;
    const double dab = s.rec_d[t];
    s.lrow[k] = s.D[(size_t)last * n + k];
    if (k == keep) {
        const double Ra = s.rec_ra[t], Rb = s.rec_rb[t];
        s.R[keep] = ((Ra + Rb) - ((double)r * dab)) * 0.5;
        return;
    }
    if (k == ret) return;
    const double sum = s.D[(size_t)sa * n + k] + s.D[(size_t)sb * n + k];
    const double duk = (sum - dab) * 0.5;
    s.urow[k] = duk;
    s.R[k == last ? ret : k] = (s.R[k] - sum) + duk;
}

// BIONJ's rows: the same slots, both matrices, the scalars of the join from the header
__global__ __launch_bounds__(256) void bionj_rows_kernel(State s, size_t n, unsigned r)
{
    const unsigned k = blockIdx.x * 256 + threadIdx.x;
    if (k >= r) return;
    const Hdr *h = s.hdr;
    const unsigned sa = h->sa, sb = h->sb, keep = sa < sb ? sa : sb, ret = sa < sb ? sb : sa, last = r - 1;
    s.lrow[k] = s.D[(size_t)last * n + k];
    s.vlrow[k] = s.V[(size_t)last * n + k];
    if (k == keep) { s.R[keep] = h->ru; s.RV[keep] = h->rvu; return; }
    if (k == ret) return;
    const double lam = h->lam, mu = h->mu;
    const double dak = s.D[(size_t)sa * n + k], dbk = s.D[(size_t)sb * n + k], vak = s.V[(size_t)sa * n + k], vbk = s.V[(size_t)sb * n + k];
    const double duk = (lam * (dak - h->la)) + (mu * (dbk - h->lb));
    const double vuk = ((lam * vak) + (mu * vbk)) - h->lmv;
    s.urow[k] = duk;
    s.vurow[k] = vuk;
    const unsigned to = k == last ? ret : k;
    s.R[to] = (s.R[k] - (dak + dbk)) + duk;
    s.RV[to] = (s.RV[k] - (vak + vbk)) + vuk;
}

// slot j of the new, (r - 1) x (r - 1) block of one matrix M from its two scratch rows
__device__ __forceinline__ void commit_cells(double *M, const double *urow, const double *lrow, size_t n, unsigned j, unsigned keep, unsigned ret,
                                             unsigned last)
{
    const bool inner = j != keep && j != ret;                        // the column cells of keep and ret are their rows' cells
    const double uv = j == keep ? 0.0 : urow[j == ret ? last : j];
    M[(size_t)keep * n + j] = uv;
    if (inner) M[(size_t)j * n + keep] = uv;
    if (ret != last) {
        const double mv = j == ret ? 0.0 : j == keep ? urow[last] : lrow[j];
        M[(size_t)ret * n + j] = mv;
        if (inner) M[(size_t)j * n + ret] = mv;
    }
}

template <bool BIONJ>
__global__ __launch_bounds__(256) void nj_commit_kernel(State s, size_t n, unsigned r, unsigned t)
{
    const unsigned j = blockIdx.x * 256 + threadIdx.x;              // a slot of the new, (r - 1) x (r - 1) block
    if (j + 1 >= r) return;
    const unsigned sa = s.hdr->sa, sb = s.hdr->sb, keep = sa < sb ? sa : sb, ret = sa < sb ? sb : sa, last = r - 1;
    commit_cells(s.D, s.urow, s.lrow, n, j, keep, ret, last);
    if (BIONJ) commit_cells(s.V, s.vurow, s.vlrow, n, j, keep, ret, last);
    if (j == 0) {
        const unsigned moved = s.ids[last];
        s.ids[keep] = (unsigned)n + t;
        if (ret != last) s.ids[ret] = moved;
    }
}

// the last three nodes by id with D_xy, D_xz, D_yz (n = 2: the two leaves and D_01)
__global__ void nj_final_kernel(State s, size_t n)
{
    if (threadIdx.x || blockIdx.x) return;
    Hdr *h = s.hdr;
    for (int q = 0; q < 3; q++) { h->last_ids[q] = NO_VERTEX; h->last_d[q] = 0.0; }
    if (n == 2) { h->last_ids[0] = 0; h->last_ids[1] = 1; h->last_d[0] = s.D[1]; }
    if (n >= 3) {
        unsigned o[3] = {0, 1, 2};
        for (int p = 0; p < 2; p++)
            for (int q = 0; q + 1 < 3 - p; q++)
                if (s.ids[o[q]] > s.ids[o[q + 1]]) { const unsigned x = o[q]; o[q] = o[q + 1]; o[q + 1] = x; }
        for (int q = 0; q < 3; q++) h->last_ids[q] = s.ids[o[q]];
        h->last_d[0] = s.D[(size_t)o[0] * n + o[1]];
        h->last_d[1] = s.D[(size_t)o[0] * n + o[2]];
        h->last_d[2] = s.D[(size_t)o[1] * n + o[2]];
    }
    h->ran = 1;
}

static int load_cells(const char *who, void *state, size_t n, const void *src, const uint32_t *ncomp, size_t ld, size_t row_begin,
                      size_t row_end, int kind, hipStream_t stream)
{
    if (!state || !src) { set_error(std::string(who) + ": NULL argument"); return TRACS_E_ARG; }
    if (kind == 1 && !ncomp) { set_error(std::string(who) + ": the per-site distance needs ncomp"); return TRACS_E_ARG; }
    if (ld < n || row_begin > row_end || row_end > n) { set_error(std::string(who) + ": rows or leading dimension outside the matrix"); return TRACS_E_ARG; }
    DeviceCall guard(stream);
    State s(state, n);
    if (row_begin == row_end || n < 2) return TRACS_OK;
    const dim3 grid(grid_for(n, 64), (unsigned)std::min<size_t>(row_end - row_begin, 4096));
    auto kernel = kind == 0 ? nj_load_kernel<0> : kind == 1 ? nj_load_kernel<1> : nj_load_kernel<2>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, s, n, src, ncomp, ld, row_begin, row_end);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

// The row sums and the n - 3 joins, enqueued.  bionj: the state has tracs_bionj_state_bytes(n) bytes (the caller's word, as the size of
// every state is); V <- D and RV <- R are two device copies, bit for bit, before the first scan.
static int run_joins(const char *who, void *state, size_t n, bool bionj, hipStream_t stream)
{
    if (!state) { set_error(std::string(who) + ": NULL state"); return TRACS_E_ARG; }
    if (n > NJ_MAX_NODES) { set_error(std::string(who) + ": more than 2^24 leaves"); return TRACS_E_ARG; }
    DeviceCall guard(stream);
    State s(state, n, nullptr, bionj);
    Hdr h{};
    int rc;
    if ((rc = read_state_header(s.hdr, n, who, stream, &h))) return rc;
    if (h.ran) { set_error(std::string(who) + ": the state has been run; initialise and load it again"); return TRACS_E_ARG; }
    if (n == 0) return TRACS_OK;
    hipLaunchKernelGGL(nj_rowsum_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, s, n);
    TRACS_HIP_CHECK(hipGetLastError());
    if (bionj && n > 3) {
        TRACS_HIP_CHECK(hipMemcpyAsync(s.V, s.D, n * n * 8, hipMemcpyDeviceToDevice, stream));
        TRACS_HIP_CHECK(hipMemcpyAsync(s.RV, s.R, n * 8, hipMemcpyDeviceToDevice, stream));
    }
    for (size_t r = n; r > 3; r--) {
        const unsigned t = (unsigned)(n - r), blocks = (unsigned)((r + 255) / 256);
        const size_t tiles = (r / 2) * ((r + NJ_TILE - 1) / NJ_TILE);
        const dim3 scan_grid((unsigned)std::min<size_t>(tiles, NJ_SCAN_BLOCKS));
        if (bionj) {
            hipLaunchKernelGGL(nj_scan_kernel<true>, scan_grid, dim3(256), 0, stream, s, n, (unsigned)r, t);
            hipLaunchKernelGGL(bionj_rows_kernel, dim3(blocks), dim3(256), 0, stream, s, n, (unsigned)r);
            hipLaunchKernelGGL(nj_commit_kernel<true>, dim3(blocks), dim3(256), 0, stream, s, n, (unsigned)r, t);
        } else {
            hipLaunchKernelGGL(nj_scan_kernel<false>, scan_grid, dim3(256), 0, stream, s, n, (unsigned)r, t);
            hipLaunchKernelGGL(nj_rows_kernel, dim3(blocks), dim3(256), 0, stream, s, n, (unsigned)r, t);
            hipLaunchKernelGGL(nj_commit_kernel<false>, dim3(blocks), dim3(256), 0, stream, s, n, (unsigned)r, t);
        }
        TRACS_HIP_CHECK(hipGetLastError());                      // (a failed launch ends the loop: nothing more is enqueued)
    }
    hipLaunchKernelGGL(nj_final_kernel, dim3(1), dim3(64), 0, stream, s, n);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

}  // namespace

extern "C" {

size_t tracs_nj_state_bytes(size_t n) { return n > NJ_MAX_NODES ? 0 : arena_bytes<State>(n); }

int tracs_nj_init(void *state, size_t n, void *stream_)
{
    if (!state) { set_error("tracs_nj_init: NULL state"); return TRACS_E_ARG; }
    if (n > NJ_MAX_NODES) { set_error("tracs_nj_init: more than 2^24 leaves"); return TRACS_E_ARG; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceCall guard(stream);
    State s(state, n);
    Hdr h0{};
    h0.n = (unsigned long long)n;
    h0.zero_pair = KEY_NONE;
    TRACS_HIP_CHECK(hipMemcpyAsync(s.hdr, &h0, sizeof(h0), hipMemcpyHostToDevice, stream));
    TRACS_HIP_CHECK(hipMemsetAsync(s.D, 0, std::max<size_t>(n, 1) * std::max<size_t>(n, 1) * 8, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));           // (h0 lives on this frame)
    return TRACS_OK;
}

int tracs_nj_load_panel(void *state, size_t n, const uint32_t *dist, const uint32_t *ncomp, size_t ld, size_t row_begin, size_t row_end,
                        int kind, void *stream)
{
    if (kind != 0 && kind != 1) { set_error("tracs_nj_load_panel: kind must be 0 (snp) or 1 (per-site)"); return TRACS_E_ARG; }
    return load_cells("tracs_nj_load_panel", state, n, dist, ncomp, ld, row_begin, row_end, kind, static_cast<hipStream_t>(stream));
}

int tracs_nj_load_f64(void *state, size_t n, const double *matrix, size_t ld, void *stream)
{
    return load_cells("tracs_nj_load_f64", state, n, matrix, nullptr, ld, 0, n, 2, static_cast<hipStream_t>(stream));
}

int tracs_nj_run(void *state, size_t n, void *stream) { return run_joins("tracs_nj_run", state, n, false, static_cast<hipStream_t>(stream)); }

size_t tracs_bionj_state_bytes(size_t n)
{
    size_t bytes = 0;
    if (n <= NJ_MAX_NODES) (void)State(nullptr, n, &bytes, true);
    return bytes;
}

int tracs_bionj_run(void *state, size_t n, void *stream) { return run_joins("tracs_bionj_run", state, n, true, static_cast<hipStream_t>(stream)); }

int tracs_nj_emit(void *state, size_t n, size_t *n_joins, uint32_t *a, uint32_t *b, double *d_ab, double *r_a, double *r_b,
                  uint32_t *last_ids, double *last_d, uint32_t *zero_pair, void *stream_)
{
    if (!state || !n_joins) { set_error("tracs_nj_emit: NULL argument"); return TRACS_E_ARG; }
    *n_joins = 0;
    if (zero_pair) zero_pair[0] = zero_pair[1] = NO_VERTEX;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceCall guard(stream);
    State s(state, n);
    Hdr h{};
    int rc;
    if ((rc = read_state_header(s.hdr, n, "tracs_nj_emit", stream, &h))) return rc;
    if (h.zero_pair != KEY_NONE) {
        const unsigned i = (unsigned)(h.zero_pair >> 32), j = (unsigned)(h.zero_pair & 0xffffffffu);
        if (zero_pair) { zero_pair[0] = i; zero_pair[1] = j; }
        set_error("tracs_nj_emit: samples " + std::to_string(i) + " and " + std::to_string(j) + " were compared over 0 sites: no per-site distance");
        return TRACS_E_ARG;
    }
    if (n && !h.ran) { set_error("tracs_nj_emit: the state has not been run"); return TRACS_E_ARG; }
    const size_t nj = n > 3 ? n - 3 : 0;
    *n_joins = nj;
    if (nj) {
        if (a) TRACS_HIP_CHECK(hipMemcpyAsync(a, s.rec_a, nj * 4, hipMemcpyDeviceToHost, stream));
        if (b) TRACS_HIP_CHECK(hipMemcpyAsync(b, s.rec_b, nj * 4, hipMemcpyDeviceToHost, stream));
        if (d_ab) TRACS_HIP_CHECK(hipMemcpyAsync(d_ab, s.rec_d, nj * 8, hipMemcpyDeviceToHost, stream));
        if (r_a) TRACS_HIP_CHECK(hipMemcpyAsync(r_a, s.rec_ra, nj * 8, hipMemcpyDeviceToHost, stream));
        if (r_b) TRACS_HIP_CHECK(hipMemcpyAsync(r_b, s.rec_rb, nj * 8, hipMemcpyDeviceToHost, stream));
    }
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    for (int q = 0; q < 3; q++) {
        if (last_ids) last_ids[q] = n ? h.last_ids[q] : NO_VERTEX;
        if (last_d) last_d[q] = n ? h.last_d[q] : 0.0;
    }
    return TRACS_OK;
}

// ---- the tree on the host: branch lengths from the records, Newick and the edge rows --------------------------------------------------
// l_a = D_ab / 2 + (R_a - R_b) / (2 (r - 2)), l_b = D_ab - l_a, one rounding per operation; the final node's three lengths from the
// last three distances.  Edges in creation order: join t gives (n + t, a), (n + t, b); the final node 2n - 3 its three children by id.
int tracs_nj_edges(size_t n, const uint32_t *a, const uint32_t *b, const double *d_ab, const double *r_a, const double *r_b,
                   const uint32_t *last_ids, const double *last_d, uint32_t *parent, uint32_t *child, double *length, size_t *n_edges)
{
    if (!n_edges) { set_error("tracs_nj_edges: NULL argument"); return TRACS_E_ARG; }
    *n_edges = 0;
    if (n < 2) return TRACS_OK;
    if (!last_ids || !last_d || !parent || !child || !length || (n > 3 && (!a || !b || !d_ab || !r_a || !r_b))) {
        set_error("tracs_nj_edges: NULL argument");
        return TRACS_E_ARG;
    }
    if (n == 2) {                                       // one edge between the two leaves
        parent[0] = last_ids[0]; child[0] = last_ids[1]; length[0] = last_d[0];
        *n_edges = 1;
        return TRACS_OK;
    }
    size_t e = 0;
    for (size_t t = 0; t + 3 < n; t++) {
        const double r = (double)(n - t);
        const double half = 0.5 * d_ab[t], diff = r_a[t] - r_b[t], den = 2.0 * (r - 2.0);
        const double quot = diff / den;
        const double la = half + quot;
        const double lb = d_ab[t] - la;
        parent[e] = (uint32_t)(n + t); child[e] = a[t]; length[e++] = la;
        parent[e] = (uint32_t)(n + t); child[e] = b[t]; length[e++] = lb;
    }
    const uint32_t top = (uint32_t)(2 * n - 3);
    const double dxy = last_d[0], dxz = last_d[1], dyz = last_d[2];
    const double lx = ((dxy + dxz) - dyz) * 0.5, ly = ((dxy + dyz) - dxz) * 0.5, lz = ((dxz + dyz) - dxy) * 0.5;
    parent[e] = top; child[e] = last_ids[0]; length[e++] = lx;
    parent[e] = top; child[e] = last_ids[1]; length[e++] = ly;
    parent[e] = top; child[e] = last_ids[2]; length[e++] = lz;
    *n_edges = e;
    return TRACS_OK;
}

}  // extern "C"

namespace {

// the shortest decimal form that reads back to the same double
void append_length(std::string &out, double x)
{
    char buf[40];
    if (std::isnan(x)) { out += "nan"; return; }
    if (std::isinf(x)) { out += x < 0 ? "-inf" : "inf"; return; }
    const auto r = std::to_chars(buf, buf + sizeof buf, x);
    out.append(buf, (size_t)(r.ptr - buf));
}

// a Newick label: quoted when it holds one of ()[]':;, or whitespace, with ' doubled
void append_label(std::string &out, const char *name)
{
    bool quote = *name == 0;
    for (const char *p = name; *p && !quote; p++)
        quote = std::strchr("()[]':;,", *p) != nullptr || *p == ' ' || (*p >= '\t' && *p <= '\r');
    if (!quote) { out += name; return; }
    out.push_back('\'');
    for (const char *p = name; *p; p++) { if (*p == '\'') out.push_back('\''); out.push_back(*p); }
    out.push_back('\'');
}

}  // namespace

// the header of the edge file whose rows tree_write_body writes under the same columns: the fields in the row loop's order
std::string tracs::tree_edges_header(const TreeColumns &cols)
{
    return std::string("parent,child,length,") + (cols.changes ? "changes," : "") + (cols.filtered ? "filtered," : "") +
           (cols.support ? "support," : "") + (cols.transfer ? "transfer," : "") + "MSA file\n";
}

// One Newick line appended to `path` and, with edges_path, the rows parent,child,length,MSA file (internal node n + t is "#t+1").
// The edges are tracs_nj_edges's: a node's children are consecutive rows, in id order; the last row's parent is the top node.  The
// writer walks the tree with a stack of its own: a caterpillar is n deep.
// cols (common.h): the labels of the internal nodes and the further fields of the edge rows.
static int tree_write_body(const char *who, const char *const *names, size_t n, const uint32_t *parent, const uint32_t *child, const double *length,
                           size_t n_edges, const TreeColumns &cols, const char *path, const char *ref, const char *edges_path)
{
    constexpr uint32_t NO_SUPPORT = 0xFFFFFFFFu;
    if (!path || (n && !names) || (n_edges && (!parent || !child || !length)) || (edges_path && !ref)) {
        set_error(std::string(who) + ": NULL argument");
        return TRACS_E_ARG;
    }
    const size_t want = n >= 3 ? 2 * n - 3 : (n == 2 ? 1 : 0);
    if (n_edges != want) { set_error(std::string(who) + ": a tree over n leaves has 2n - 3 edges"); return TRACS_E_ARG; }
    const size_t n_nodes = n >= 3 ? 2 * n - 2 : n;
    std::string text;
    if (n == 1) append_label(text, names[0]);
    else if (n == 2) {
        const double half = length[0] * 0.5;
        text.push_back('(');
        append_label(text, names[parent[0]]); text.push_back(':'); append_length(text, half); text.push_back(',');
        append_label(text, names[child[0]]); text.push_back(':'); append_length(text, half); text.push_back(')');
    } else if (n >= 3) {
        // first[p], count[p]: the rows of p's children; up[c]: the row that hangs c under its parent
        std::vector<size_t> first(n_nodes, 0), up(n_nodes, (size_t)-1);
        std::vector<uint32_t> count(n_nodes, 0);
        for (size_t e = 0; e < n_edges; e++) {
            const uint32_t p = parent[e], c = child[e];
            if (p < n || p >= n_nodes || c >= n_nodes || c == p || up[c] != (size_t)-1 || (count[p] && first[p] + count[p] != e)) {
                set_error(std::string(who) + ": the edges are not a tree in creation order");
                return TRACS_E_ARG;
            }
            if (!count[p]) first[p] = e;
            count[p]++;
            up[c] = e;
        }
        const uint32_t top = parent[n_edges - 1];
        struct Frame { uint32_t node, next; };
        std::vector<Frame> stack;
        stack.push_back({top, 0});
        text.push_back('(');
        while (!stack.empty()) {
            Frame &f = stack.back();
            if (f.next == count[f.node]) {                           // the node is complete
                const uint32_t node = f.node;
                stack.pop_back();
                text.push_back(')');
                if (node != top) {
                    if (cols.transfer) { if (!std::isnan(cols.transfer[up[node]])) append_length(text, cols.transfer[up[node]]); }
                    else if (cols.support && cols.support[up[node]] != NO_SUPPORT) text += std::to_string(cols.support[up[node]]);
                    text.push_back(':');
                    append_length(text, length[up[node]]);
                }
                continue;
            }
            if (f.next) text.push_back(',');
            const size_t e = first[f.node] + f.next++;
            const uint32_t c = child[e];
            if (c < n) { append_label(text, names[c]); text.push_back(':'); append_length(text, length[e]); }
            else if (!count[c]) { set_error(std::string(who) + ": an internal node without children"); return TRACS_E_ARG; }
            else { text.push_back('('); stack.push_back({c, 0}); }
        }
    }
    if (n) {
        text += ";\n";
        std::FILE *fh = std::fopen(path, "ab");
        if (!fh) { set_error(std::string("cannot open ") + path + " for appending"); return TRACS_E_OPEN; }
        const bool ok = std::fwrite(text.data(), 1, text.size(), fh) == text.size();
        if (std::fclose(fh) != 0 || !ok) { set_error(std::string("write to ") + path + " failed"); return TRACS_E_OPEN; }
    }
    if (edges_path) {
        std::string rows;
        auto node_name = [&](uint32_t v) {
            if (v < n) rows += names[v];
            else { rows.push_back('#'); rows += std::to_string((size_t)v - n + 1); }
        };
        for (size_t e = 0; e < n_edges; e++) {
            node_name(parent[e]); rows.push_back(',');
            node_name(child[e]); rows.push_back(',');
            append_length(rows, length[e]); rows.push_back(',');
            if (cols.changes) { rows += std::to_string(cols.changes[e]); rows.push_back(','); }
            if (cols.filtered) { rows += std::to_string(cols.filtered[e]); rows.push_back(','); }
            if (cols.support) {
                if (child[e] >= n && n >= 3 && cols.support[e] != NO_SUPPORT) rows += std::to_string(cols.support[e]);
                else rows += "NA";
                rows.push_back(',');
            }
            if (cols.transfer) {
                if (child[e] >= n && n >= 3 && !std::isnan(cols.transfer[e])) append_length(rows, cols.transfer[e]);
                else rows += "NA";
                rows.push_back(',');
            }
            rows += ref; rows.push_back('\n');
        }
        std::FILE *fh = std::fopen(edges_path, "ab");
        if (!fh) { set_error(std::string("cannot open ") + edges_path + " for appending"); return TRACS_E_OPEN; }
        const bool ok = rows.empty() || std::fwrite(rows.data(), 1, rows.size(), fh) == rows.size();
        if (std::fclose(fh) != 0 || !ok) { set_error(std::string("write to ") + edges_path + " failed"); return TRACS_E_OPEN; }
    }
    return TRACS_OK;
}

extern "C" {

int tracs_tree_write(const char *const *names, size_t n, const uint32_t *parent, const uint32_t *child, const double *length, size_t n_edges,
                     const char *path, const char *ref, const char *edges_path)
{
    return tree_write_body("tracs_tree_write", names, n, parent, child, length, n_edges, {nullptr, nullptr, nullptr, nullptr}, path, ref, edges_path);
}

// tests: tree_edges_header for the columns that are named (non-zero) into out[cap]
int tracs_debug_tree_edges_header(int support, int transfer, int changes, int filtered, char *out, size_t cap)
{
    static const uint32_t u = 0;
    static const double d = 0.0;
    const std::string head = tree_edges_header({support ? &u : nullptr, transfer ? &d : nullptr, changes ? &u : nullptr, filtered ? &u : nullptr});
    if (!out || cap <= head.size()) { set_error("tracs_debug_tree_edges_header: the buffer is too small"); return TRACS_E_ARG; }
    std::memcpy(out, head.c_str(), head.size() + 1);
    return TRACS_OK;
}

// tracs_tree_write with the number of changes on every edge: the same Newick line, and the rows
// parent,child,length,changes,ref.
int tracs_tree_write_changes(const char *const *names, size_t n, const uint32_t *parent, const uint32_t *child, const double *length,
                             size_t n_edges, const uint32_t *changes, const char *path, const char *ref, const char *edges_path)
{
    if (n_edges && !changes) { set_error("tracs_tree_write_changes: NULL argument"); return TRACS_E_ARG; }
    return tree_write_body("tracs_tree_write_changes", names, n, parent, child, length, n_edges, {nullptr, nullptr, changes, nullptr}, path, ref, edges_path);
}

// tracs_tree_write_changes with the changes the branch filter keeps on every edge: the same Newick line, and the rows
// parent,child,length,changes,filtered,ref.
int tracs_tree_write_filtered(const char *const *names, size_t n, const uint32_t *parent, const uint32_t *child, const double *length,
                              size_t n_edges, const uint32_t *changes, const uint32_t *filtered, const char *path, const char *ref,
                              const char *edges_path)
{
    if (n_edges && (!changes || !filtered)) { set_error("tracs_tree_write_filtered: NULL argument"); return TRACS_E_ARG; }
    return tree_write_body("tracs_tree_write_filtered", names, n, parent, child, length, n_edges, {nullptr, nullptr, changes, filtered}, path, ref, edges_path);
}

// tracs_tree_write with bootstrap support: `(A:1,B:2)87:0.5`, and the rows parent,child,length,support,ref.
int tracs_tree_write_support(const char *const *names, size_t n, const uint32_t *parent, const uint32_t *child, const double *length,
                             size_t n_edges, const uint32_t *support, uint32_t replicates, const char *path, const char *ref, const char *edges_path)
{
    if (n_edges && !support) { set_error("tracs_tree_write_support: NULL argument"); return TRACS_E_ARG; }
    static const uint32_t none = 0xFFFFFFFFu;
    for (size_t e = 0; e < n_edges; e++)
        if (support[e] != none && support[e] > replicates) {
            set_error("tracs_tree_write_support: a support of " + std::to_string(support[e]) + " out of " + std::to_string(replicates) + " replicates");
            return TRACS_E_ARG;
        }
    return tree_write_body("tracs_tree_write_support", names, n, parent, child, length, n_edges, {support, nullptr, nullptr, nullptr}, path, ref, edges_path);
}

// tracs_tree_write_support with the transfer support as the label: x_e = 1 - Phi_e / (B (p_e - 1)), one rounding per
// operation, on the host; `(A:1,B:2)0.875:0.5`, and the rows parent,child,length,support,transfer,ref.
int tracs_tree_write_transfer(const char *const *names, size_t n, const uint32_t *parent, const uint32_t *child, const double *length,
                              size_t n_edges, const uint32_t *support, const uint64_t *sum_phi, const uint32_t *light, uint32_t replicates,
                              const char *path, const char *ref, const char *edges_path)
{
    if (n_edges && (!support || !sum_phi || !light || !child)) { set_error("tracs_tree_write_transfer: NULL argument"); return TRACS_E_ARG; }
    if (replicates < 1) { set_error("tracs_tree_write_transfer: at least one replicate"); return TRACS_E_ARG; }
    static const uint32_t none = 0xFFFFFFFFu;
    std::vector<double> x(std::max<size_t>(n_edges, 1), std::nan(""));
    for (size_t e = 0; e < n_edges; e++) {
        if (support[e] != none && support[e] > replicates) {
            set_error("tracs_tree_write_transfer: a support of " + std::to_string(support[e]) + " out of " + std::to_string(replicates) + " replicates");
            return TRACS_E_ARG;
        }
        if (n < 4 || child[e] < n) continue;
        const uint64_t den = (uint64_t)replicates * (uint64_t)(light[e] - 1u);
        if (light[e] < 2 || light[e] > n / 2 || sum_phi[e] > den) {
            set_error("tracs_tree_write_transfer: edge " + std::to_string(e) + " has the sum " + std::to_string(sum_phi[e]) + " over " +
                      std::to_string(replicates) + " replicates with a lighter side of " + std::to_string(light[e]) + " leaves");
            return TRACS_E_ARG;
        }
        const double q = (double)sum_phi[e] / (double)den;
        x[e] = 1.0 - q;
    }
    return tree_write_body("tracs_tree_write_transfer", names, n, parent, child, length, n_edges, {support, x.data(), nullptr, nullptr}, path, ref, edges_path);
}

}  // extern "C"
