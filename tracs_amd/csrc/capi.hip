// capi.hip -- library-wide state (error slot, scratch pool) and the host-level pairsnp entry.
//
// tracs_pairsnp restates the DRIVER part of /root/reference/src/pairsnp.hpp:320-457:
// argument check (:340-343), one- vs two-file pair ranges (:352-360), the output tuple (:451-457).
// The arithmetic is in pairsnp.hip.
#include "common.h"
#include "fasta.h"
#include "rowwriter.h"
#include "debug_api.h"
#include "alloc_path.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

namespace tracs {

static thread_local std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }

struct Scratch { void *ptr = nullptr; size_t bytes = 0; };
static Scratch g_scratch[8][WS_SLOT_COUNT];
static std::mutex g_scratch_mu;
// diagnostics (tracs_debug_poison_scratch / tracs_debug_scratch_hits): the byte every outermost DeviceCall fills the device's slots
// with (-1: off), and how often each slot has been handed out since the counts were last read
static std::atomic<int> g_poison{-1};         // (relaxed: a tests-only switch, read once per DeviceCall)
static uint64_t g_slot_hits[WS_SLOT_COUNT];

int workspace_bytes(WsSlot slot, size_t bytes, void **out)
{
    int dev = 0;
    TRACS_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 8 || slot < 0 || slot >= WS_SLOT_COUNT) { set_error("workspace_get: bad device/slot"); return TRACS_E_ARG; }
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    Scratch &s = g_scratch[dev][slot];
    g_slot_hits[slot]++;
    if (s.bytes < bytes) {
        if (s.ptr) { TRACS_HIP_CHECK(hipDeviceSynchronize()); device_free(s.ptr); s.ptr = nullptr; s.bytes = 0; }
        const size_t want = bytes + bytes / 4 + 256;
        if (const int rc = device_alloc(want, "workspace", &s.ptr)) return rc;
        s.bytes = want;
        if (const int poison = g_poison.load(std::memory_order_relaxed); poison >= 0) {      // growth inside a call: the new buffer starts as the rest of the pool did
            TRACS_HIP_CHECK(hipMemset(s.ptr, poison, s.bytes));
            TRACS_HIP_CHECK(hipDeviceSynchronize());
        }
    }
    *out = s.ptr;
    return TRACS_OK;
}

static std::recursive_mutex g_call_mu[8];
static hipStream_t g_last_stream[8];
static bool g_have_stream[8];
static int g_call_depth[8];                      // DeviceCalls the owning thread holds on the device (under g_call_mu)
static bool g_caller_orders_streams = false;     // tracs_set_stream_policy

// every allocated slot of `dev` <- the poison byte, with the device drained before and after (the outermost DeviceCall, poison on)
static void poison_scratch(int dev, int byte)
{
    (void)hipDeviceSynchronize();
    {
        std::lock_guard<std::mutex> lock(g_scratch_mu);
        for (Scratch &s : g_scratch[dev])
            if (s.ptr) (void)hipMemset(s.ptr, byte, s.bytes);
    }
    (void)hipDeviceSynchronize();
}

DeviceCall::DeviceCall(hipStream_t stream) : dev(0)
{
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 8) dev = 0;
    g_call_mu[dev].lock();
    if (g_have_stream[dev] && g_last_stream[dev] != stream && !g_caller_orders_streams) (void)hipDeviceSynchronize();
    g_last_stream[dev] = stream;
    g_have_stream[dev] = true;
    const int poison = g_poison.load(std::memory_order_relaxed);
    if (g_call_depth[dev]++ == 0 && poison >= 0) poison_scratch(dev, poison);
}
DeviceCall::~DeviceCall()
{
    g_call_depth[dev]--;
    g_call_mu[dev].unlock();
}

void workspace_release_all()
{
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    for (auto &dev : g_scratch)
        for (auto &s : dev)
            if (s.ptr) { device_free(s.ptr); s.ptr = nullptr; s.bytes = 0; }
}

}  // namespace tracs

using namespace tracs;

void tracs_debug_poison_scratch(int byte)
{
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    g_poison.store(byte >= 0 && byte <= 255 ? byte : -1, std::memory_order_relaxed);
}

size_t tracs_debug_scratch_hits(uint64_t *hits, size_t room)
{
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    for (size_t s = 0; s < (size_t)WS_SLOT_COUNT; s++) {
        if (hits && s < room) hits[s] = g_slot_hits[s];
        g_slot_hits[s] = 0;
    }
    return (size_t)WS_SLOT_COUNT;
}

// The allocation path's counters (alloc_path.h).  out[4] <- live device blocks, live device bytes, live pinned blocks and the allocations
// (device or pinned, failed ones included) since the last reading; reading resets the fourth.
void tracs_debug_alloc_stats(uint64_t *out) { alloc_stats(out); }
// The nth allocation from now (1-based, device or pinned) fails as out of memory without reaching HIP.  One shot; 0 turns it off.
void tracs_debug_fail_alloc(long nth) { fail_alloc(nth); }

// TRACS_STAGE_TRACE=1: wall time of the stages of the host-level entry points on stderr, one "[stage] name seconds" line each
// (scripts/bench_e2e.py collects them into the end-to-end table of DESIGN.md 5)
struct StageClock {
    bool on;
    std::chrono::steady_clock::time_point t;
    StageClock() : on(sw::is_set(sw::TRACS_STAGE_TRACE)), t(std::chrono::steady_clock::now()) {}
    void mark(const char *name, double bytes = 0.0)
    {
        if (!on) return;
        (void)hipDeviceSynchronize();
        const auto now = std::chrono::steady_clock::now();
        const double s = std::chrono::duration<double>(now - t).count();
        if (bytes > 0.0) std::fprintf(stderr, "[stage] %s %.4f s (%.2f GB/s)\n", name, s, bytes / s / 1e9);
        else std::fprintf(stderr, "[stage] %s %.4f s\n", name, s);
        t = std::chrono::steady_clock::now();
    }
    void memory(const char *when)                                     // "[memory] when N MiB": what the device has in use, by every process
    {
        size_t idle = 0, all = 0;
        if (on && hipMemGetInfo(&idle, &all) == hipSuccess) std::fprintf(stderr, "[memory] %s %.1f MiB\n", when, (double)(all - idle) / 1048576.0);
    }
};
// the time since the clock's last mark or lap goes into `acc` (the entry points that print sums over their panels)
static void lap(StageClock &clock, double &acc)
{
    if (!clock.on) return;
    (void)hipDeviceSynchronize();
    const auto now = std::chrono::steady_clock::now();
    acc += std::chrono::duration<double>(now - clock.t).count();
    clock.t = now;
}

// dst[base + t] = src[t] (uint32 -> uint64) on several host threads: at 5 x 10^7 pairs the five result columns are 2 GB
static void widen_append(std::vector<uint64_t> &dst, const unsigned *src, size_t count)
{
    const size_t base = dst.size();
    dst.resize(base + count);
    uint64_t *out = dst.data() + base;
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const size_t nthr = count < (1u << 20) ? 1 : hw;
    if (nthr == 1) { for (size_t t = 0; t < count; t++) out[t] = src[t]; return; }
    std::vector<std::thread> pool;
    const size_t per = (count + nthr - 1) / nthr;
    for (size_t k = 0; k < nthr; k++) {
        const size_t b = k * per, e = std::min(count, b + per);
        if (b < e) pool.emplace_back([=]() { for (size_t t = b; t < e; t++) out[t] = src[t]; });
    }
    for (auto &th : pool) th.join();
}

// Ctrl-C during tracs_pairsnp (src/pairsnp.hpp:21-25,326,385-388,434-441: the reference installs its own SIGINT handler, lets
// the loop drain, prints "Interrupted by user!" and exit(1)s).  Here the handler only lives for the duration of the call, the
// panel loop looks at the flag between row panels (a running kernel cannot be stopped: <= one panel, ~0.4 s at 10 000 x 5 Mbp),
// and the call returns TRACS_E_INTERRUPTED with the reference's message; the Python layer raises KeyboardInterrupt.
static volatile sig_atomic_t g_sigint = 0;
static void on_sigint(int) { g_sigint = 1; }
struct SigintScope {
    struct sigaction old;
    bool installed;
    SigintScope()
    {
        g_sigint = 0;
        struct sigaction sa;
        std::memset(&sa, 0, sizeof(sa));
        sa.sa_handler = on_sigint;
        sigemptyset(&sa.sa_mask);
        installed = sigaction(SIGINT, &sa, &old) == 0;
    }
    ~SigintScope() { if (installed) (void)sigaction(SIGINT, &old, nullptr); }
};

// What a sample rule saw: every record read, its N sites among the columns the file rules leave, whether it stayed.
// Without a sample rule `names` is empty and the accessors answer from the loaded samples: all kept, counts 0.
struct SourceSamples {
    std::vector<std::string> names;
    std::vector<uint32_t> n_count;
    std::vector<uint8_t> kept;
    size_t rule_sites = 0;               // L': the columns the file rules leave (every column without file rules)
};

struct tracs_pairsnp_result {
    size_t nseq = 0, L = 0;
    std::vector<uint64_t> rows, cols, dist, filt, ncomp;
    std::vector<std::string> names;
    SourceSamples source;
};

// the date difference of every emitted pair, as tracs/transcluster.py:26-33 takes it: |t_i - t_j| / 31556952.0 with t = whole days in seconds
extern "C" __global__ __launch_bounds__(256) void coo_delta_kernel(const unsigned *__restrict__ rows, const unsigned *__restrict__ cols,
                                                                   const int *__restrict__ days, size_t n, double *__restrict__ out)
{
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (size_t)gridDim.x * 256) {
        const long long dd = (long long)days[rows[t]] - (long long)days[cols[t]];
        out[t] = (double)((dd < 0 ? -dd : dd) * 86400ll) / 31556952.0;
    }
}

// ---- what the host entry points below share: owners, the row-panel walk, the pair-extraction stage ------------------------------------
namespace {

// the copy stream of tracs_distance_run and its events; declared AFTER the pinned buffers it copies into, so that it is drained and
// destroyed before they are freed
struct CopyLane {
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr}, ready = nullptr;
    CopyLane() = default;
    CopyLane(const CopyLane &) = delete;
    CopyLane &operator=(const CopyLane &) = delete;
    int create()
    {
        TRACS_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        for (auto &e : ev) TRACS_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        TRACS_HIP_CHECK(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
        return TRACS_OK;
    }
    ~CopyLane()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (ready) (void)hipEventDestroy(ready);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct ResultFree { void operator()(tracs_pairsnp_result *r) const { delete r; } };
using ResultOwner = std::unique_ptr<tracs_pairsnp_result, ResultFree>;

static int interrupted() { set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }

// where a stage-trace lap goes: the entry point that owns the timers says which of its sums takes it
enum Lap { LAP_DENSE, LAP_TC, LAP_COO, LAP_FILTER };
using LapFn = std::function<void(Lap)>;

// The row-panel walk of every host entry point: the pair range (src/pairsnp.hpp:348-360), the panel height (~1 GiB per dense uint32
// matrix; TRACS_FOREST_PANEL_ROWS: diagnostics -- small panels in tests, so that every route crosses panel boundaries), the dense
// buffers, and per panel the SIGINT look, the dense call (early out beyond `dist`) and -- directly after it, before anything reads
// the panel -- the pair rule.
struct Panel {
    size_t r0 = 0, r1 = 0;
    unsigned *bd = nullptr, *bn = nullptr;       // addressed as base[i * n + j] with i absolute: the bases are shifted by r0 rows
    double *bp = nullptr, *be = nullptr;         // the f64 panels, when the walk holds them
};

struct PanelWalk {
    tracs_alignment *a;
    size_t n, i_end, j_start;
    int dist;
    uint32_t min_sites;
    LapFn lap;
    size_t height = 0, at = 0;
    DeviceBuffer d_dist, d_nn, d_off, d_p, d_e;

    PanelWalk(tracs_alignment *a_, int n_fasta, size_t n0, int dist_, uint32_t min_sites_, LapFn lap_ = nullptr)
        : a(a_), n(a_->n), i_end(n_fasta == 1 ? a_->n : n0), j_start(n_fasta == 1 ? 0 : n0), dist(dist_), min_sites(min_sites_), lap(std::move(lap_)) {}
    bool any() const { return n >= 2 && i_end > 0 && j_start < n; }       // else: no pair exists
    int64_t *off() const { return d_off.as<int64_t>(); }
    // with_off: row offsets for a PairStage; with_f64: the P(direct) and E(K) panels of the dense transcluster route
    int begin(bool with_off, bool with_f64)
    {
        const size_t rows = (size_t)std::max(0LL, sw::integer(sw::TRACS_FOREST_PANEL_ROWS, 0LL));     // (0: not set, or below 1)
        height = rows ? std::min(rows, i_end) : std::max<size_t>(64, std::min<size_t>(i_end, (1ull << 28) / std::max<size_t>(n, 1)));
        int rc;
        if ((rc = d_dist.alloc(height * n * 4, "dist")) || (rc = d_nn.alloc(height * n * 4, "nn"))) return rc;
        if (with_off && (rc = d_off.alloc((height + 1) * 8, "off"))) return rc;
        if (with_f64 && ((rc = d_p.alloc(height * n * 8, "p")) || (rc = d_e.alloc(height * n * 8, "e")))) return rc;
        return TRACS_OK;
    }
    bool more() const { return at < i_end; }
    int next(Panel &p)
    {
        if (g_sigint) return interrupted();
        p.r0 = at;
        p.r1 = at = std::min(i_end, at + height);
        p.bd = d_dist.as<unsigned>() - p.r0 * n;
        p.bn = d_nn.as<unsigned>() - p.r0 * n;
        p.bp = d_p.ptr ? d_p.as<double>() - p.r0 * n : nullptr;
        p.be = d_e.ptr ? d_e.as<double>() - p.r0 * n : nullptr;
        int rc = tracs_pairsnp_dense_thr(a, p.r0, p.r1, j_start, p.bd, p.bn, n, dist, nullptr);
        if (!rc && min_sites) rc = pairs_min_sites(p.bd, p.bn, n, n, p.r0, p.r1, j_start, dist, min_sites, nullptr);
        if (!rc && lap) lap(LAP_DENSE);
        return rc;
    }
};

// The pairs of one panel within the threshold, in row-major order (src/pairsnp.hpp:451-455), as columns on the device.
// With dates (set_days) the columns carry P(direct) and E(K): without --filter from transcluster on the dense panel (the walk holds
// the f64 panels: begin(true, dense_tc())), with --filter from the FILTERED distance, pair by pair (tracs/distance.py:183-193 ->
// tracs/transcluster.py:8-41).  total = 0 is a result like any other: the panel holds no pair, the columns are not valid.
struct PairColumns {
    size_t total = 0;
    unsigned *rows = nullptr, *cols = nullptr, *d = nullptr, *nn = nullptr, *filt = nullptr;
    double *p = nullptr, *e = nullptr;
};

struct PairStage {
    const PanelWalk &w;
    bool filter;
    double lamb, beta, precision;
    DeviceBuffer d_days, coo, cp;

    PairStage(const PanelWalk &walk, int filter_, double lamb_ = 0.0, double beta_ = 0.0, double precision_ = 0.0)
        : w(walk), filter(filter_ != 0), lamb(lamb_), beta(beta_), precision(precision_) {}
    int set_days(const int32_t *days) { return d_days.upload(days, w.n * 4, "days"); }
    bool with_dates() const { return d_days.ptr != nullptr; }
    bool dense_tc() const { return with_dates() && !filter; }
    const int *days() const { return d_days.as<int>(); }
    void release() { coo.release(); cp.release(); }
    int extract(const Panel &pn, PairColumns &c)
    {
        c = PairColumns();
        const size_t n = w.n;
        int rc;
        if (dense_tc()) {
            if ((rc = tracs_trans_dist_dense(pn.bd, n, n, pn.r0, pn.r1, w.j_start, w.dist, days(), lamb, beta, precision, 1, pn.bp, pn.be, nullptr))) return rc;
            if (w.lap) w.lap(LAP_TC);
        }
        if ((rc = tracs_coo_count(pn.bd, n, n, pn.r0, pn.r1, w.j_start, w.dist, w.off(), nullptr))) return rc;
        long long total = 0;
        TRACS_HIP_CHECK(hipMemcpy(&total, w.off() + (pn.r1 - pn.r0), 8, hipMemcpyDeviceToHost));
        if (total <= 0) return TRACS_OK;
        const size_t t = (size_t)total;
        if ((rc = coo.grow(t * 4 * (filter ? 5 : 4), "coo"))) return rc;
        if (with_dates() && (rc = cp.grow(t * (filter ? 24 : 16), "cp"))) return rc;
        c.rows = coo.as<unsigned>(); c.cols = c.rows + t; c.d = c.rows + 2 * t; c.nn = c.rows + 3 * t;
        c.filt = filter ? c.rows + 4 * t : nullptr;
        c.p = with_dates() ? cp.as<double>() : nullptr;
        c.e = with_dates() ? c.p + t : nullptr;
        if ((rc = tracs_coo_fill(pn.bd, pn.bn, n, n, pn.r0, pn.r1, w.j_start, w.dist, w.off(), c.rows, c.cols, c.d, c.nn, nullptr))) return rc;
        if (dense_tc() && (rc = tracs_coo_fill_f64(pn.bd, n, n, pn.r0, pn.r1, w.j_start, w.dist, w.off(), pn.bp, pn.be, c.p, c.e, nullptr))) return rc;
        if (w.lap) w.lap(LAP_COO);
        if (filter) {
            // the recombination filter on the emitted pairs (src/pairsnp.hpp:405-413): SNP sites from the samples' departure lists
            if (g_sigint) return interrupted();
            if ((rc = tracs_filter_recomb_pairs(w.a, c.rows, c.cols, c.d, t, c.filt, nullptr))) return rc;
            if (with_dates()) {
                double *delta = c.p + 2 * t;
                hipLaunchKernelGGL(coo_delta_kernel, dim3((unsigned)std::min<size_t>((t + 255) / 256, 65535)), dim3(256), 0, nullptr, c.rows, c.cols,
                                   days(), t, delta);
                if ((rc = tracs_trans_dist_device(reinterpret_cast<const int32_t *>(c.filt), delta, t, lamb, beta, precision, 1, c.p, c.e, nullptr))) return rc;
            }
            if (w.lap) w.lap(LAP_FILTER);
        }
        c.total = t;
        return TRACS_OK;
    }
};

}  // namespace

extern "C" {

void tracs_set_stream_policy(int caller_orders_streams) { g_caller_orders_streams = caller_orders_streams != 0; }

const char *tracs_last_error(void) { return g_error.c_str(); }
int tracs_abi_version(void) { return 1; }

int tracs_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void tracs_free(void *p) { std::free(p); }

// host-only: parse a FASTA and return record count, length and an FNV-1a hash over names and sequences (tests)
int tracs_debug_read_fasta(const char *path, size_t *n, size_t *L, uint64_t *hash)
{
    FastaData fd;
    std::string err;
    const int rc = read_fasta(path, fd, err);
    if (rc) { set_error(err); return rc; }
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const uint8_t *b, size_t k) { for (size_t i = 0; i < k; i++) { h ^= b[i]; h *= 1099511628211ull; } };
    if (hash) {
        for (auto &nm : fd.names) { mix(reinterpret_cast<const uint8_t *>(nm.data()), nm.size()); const uint8_t z = 0; mix(&z, 1); }
        mix(fd.seq.data(), fd.seq.size());
    }
    if (n) *n = fd.n;
    if (L) *L = fd.L;
    if (hash) *hash = h;
    return TRACS_OK;
}

// The start-up of a process's first call, off the caller's thread: the HIP runtime, the device context and this library's code
// object (loaded on its first kernel launch: tens of milliseconds for ~2 MB of kernels).  `tracs distance` calls it before it reads
// its metadata and the FASTA, so a small alignment does not wait for them in tracs_distance_open.  Only with ONE visible device:
// a fresh thread's current device is 0, which is not necessarily the caller's.
__global__ void warm_up_kernel(unsigned *p) { if (p) *p = 0u; }
static void warm_up_body()
{
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd != 1) { (void)hipGetLastError(); return; }
    (void)hipFree(nullptr);
    hipLaunchKernelGGL(warm_up_kernel, dim3(1), dim3(1), 0, nullptr, (unsigned *)nullptr);
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
}
extern "C" void tracs_warm_up(void)
{
    static std::once_flag once;
    std::call_once(once, [] { std::thread(warm_up_body).detach(); });
}

// A site rule of the FASTA entry points: which columns stay.  No rule at all is a NULL pointer, and then nothing
// below differs from what the entry points did before there were rules.
struct SiteRule {
    const uint64_t *keep = nullptr;      // host bitmap over the columns read, NULL: every column may stay
    size_t keep_len = 0;
    uint32_t max_n = UINT32_MAX;         // a column stays only if at most that many samples are N there
    std::vector<uint64_t> kept;          // out: the final bitmap over the columns read
    size_t source_len = 0;               // out: columns read
    // the _rules entry points; shares < 0 and min_sites = 0: no rule
    double max_n_share = -1.0;           // max_n = floor(share x the samples that SURVIVE the sample rule), taken once they are known
    double max_sample_share = -1.0;      // a record goes when more than floor(share x L') of the file-kept columns are N in it
    uint32_t min_sites = 0;              // a pair is eligible only if it was compared over at least that many kept sites
    SourceSamples source;                // out: rule_sites always, the rest with the sample rule
    bool active() const { return keep != nullptr || max_n != UINT32_MAX; }
    bool sample_rule() const { return max_sample_share >= 0.0; }
};

static int apply_sample_rule(tracs_alignment **pa, FastaData &fd, size_t *n0, int n_fasta, SiteRule *rule);

static int alignment_from_fasta_sites(const char *const *fasta, int n_fasta, tracs_alignment **out, char **names_out,
                                      size_t *names_bytes, size_t *n_first_file, SiteRule *rule);

int tracs_alignment_from_fasta(const char *const *fasta, int n_fasta, tracs_alignment **out, char **names_out,
                               size_t *names_bytes, size_t *n_first_file)
{
    return alignment_from_fasta_sites(fasta, n_fasta, out, names_out, names_bytes, n_first_file, nullptr);
}

// read + pack, then -- only with a rule -- select the kept columns into a new handle and free the one that was packed
static int alignment_from_fasta_sites(const char *const *fasta, int n_fasta, tracs_alignment **out, char **names_out,
                                      size_t *names_bytes, size_t *n_first_file, SiteRule *rule)
{
    if (out) *out = nullptr;
    if (names_out) *names_out = nullptr;
    if (!fasta || !out || n_fasta < 1 || n_fasta > 2) { set_error("Invalid number of fasta files!"); return TRACS_E_ARG; }
    FastaData fd;
    size_t n0 = 0;
    StageClock clock;
    // the HIP runtime comes up (first call of the process: ~0.3-0.5 s) while the host threads read the text
    // (a context only where there is one device to have it on: with several visible, a fresh thread's current device is 0, not
    // necessarily the caller's -- a rank of a multi-GPU job would leave a primary context on GPU 0 --; the runtime itself still comes up)
    std::thread warm(warm_up_body);
    struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } join_warm{warm};
    for (int f = 0; f < n_fasta; f++) {
        std::string err;
        FastaData one;
        int rc = read_fasta(fasta[f], one, err);
        if (rc) { set_error(err); return rc; }
        if (f == 0) { fd = std::move(one); n0 = fd.n; }
        else {
            // load_seqs only checks lengths inside one file (pairsnp.hpp:94-98); two files of different
            // length would make the reference AND bitsets of different sizes (undefined) -- refuse.
            if (fd.n && one.n && one.L != fd.L) { set_error("Error reading FASTA, variable sequence lengths!"); return TRACS_E_RAGGED; }
            if (!fd.n) fd.L = one.L;
            fd.seq.insert(fd.seq.end(), one.seq.begin(), one.seq.end());
            fd.names.insert(fd.names.end(), one.names.begin(), one.names.end());
            fd.n += one.n;
        }
    }
    if (warm.joinable()) warm.join();
    clock.mark("read FASTA (host)", (double)fd.n * (double)fd.L);
    tracs_alignment *a = nullptr;
    int rc = tracs_alignment_create(fd.n, fd.L, &a);
    if (rc) return rc;
    clock.mark("allocate planes + arena");
    // pack in sample batches of <= 1 GiB of ASCII
    const size_t batch = fd.L ? std::max<size_t>(1, (1ull << 30) / fd.L) : fd.n;
    for (size_t s = 0; s < fd.n && fd.L; s += batch) {
        const size_t cnt = std::min(batch, fd.n - s);
        rc = tracs_alignment_pack(a, fd.seq.data() + s * fd.L, s, cnt, 0, nullptr);
        if (rc) { tracs_alignment_free(a); return rc; }
    }
    clock.mark("H2D + pack", (double)fd.n * (double)fd.L);
    if (rule) {
        rule->source_len = a->L;
        rule->source.rule_sites = a->L;
        if (rule->keep && rule->keep_len == a->L) {
            size_t lp = 0;
            for (size_t w = 0; w < (a->L + 63) / 64; w++) {
                const uint64_t m = (w == a->L / 64) ? ((1ull << (a->L & 63)) - 1) : ~0ull;
                lp += (size_t)__builtin_popcountll(rule->keep[w] & m);
            }
            rule->source.rule_sites = lp;
        }
        if (rule->sample_rule()) {
            // file rules first (the counts are taken under their bitmap), then the records, then -- below -- the N share over the survivors
            rc = apply_sample_rule(&a, fd, &n0, n_fasta, rule);
            if (rc) { tracs_alignment_free(a); return rc; }
            clock.mark("sample rule (N counts, gather)");
        }
        if (rule->max_n_share >= 0.0) rule->max_n = (uint32_t)std::floor(rule->max_n_share * (double)a->n);
        if (rule->active()) {
            // (the N rule counts over every loaded sample: both files of a two-file run)
            tracs_alignment *sel = nullptr;
            rule->kept.assign((a->L + 63) / 64, 0);
            rc = select_sites(a, rule->keep, rule->keep_len, rule->max_n, &sel, rule->kept.data(), nullptr, nullptr, true);
            tracs_alignment_free(a);
            if (rc) return rc;
            a = sel;
            clock.mark("site rules (N counts, list, selection)");
        }
    }
    if (names_out) {
        size_t bytes = 0;
        for (auto &nm : fd.names) bytes += nm.size() + 1;
        char *blk = static_cast<char *>(std::malloc(bytes ? bytes : 1));
        size_t o = 0;
        for (auto &nm : fd.names) { std::memcpy(blk + o, nm.c_str(), nm.size() + 1); o += nm.size() + 1; }
        *names_out = blk;
        if (names_bytes) *names_bytes = bytes;
    }
    if (n_first_file) *n_first_file = n0;
    *out = a;
    return TRACS_OK;
}

// The sample rule on a freshly packed handle: counts under the file rules' bitmap, the kept flags, and -- unless every record stays --
// the survivors gathered into a new handle that replaces *pa (the packed one is freed); fd.names and *n0 shrink with it.
static int apply_sample_rule(tracs_alignment **pa, FastaData &fd, size_t *n0, int n_fasta, SiteRule *rule)
{
    tracs_alignment *a = *pa;
    const size_t n = a->n;
    SourceSamples &src = rule->source;
    src.names = fd.names;
    src.n_count.assign(n, 0);
    src.kept.assign(n, 1);
    if (rule->keep && rule->keep_len != a->L) {
        set_error("site rules: the keep bitmap covers " + std::to_string(rule->keep_len) + " sites, the alignment has " + std::to_string(a->L));
        return TRACS_E_ARG;
    }
    if (!n) { set_error("no sample left after the sample rule"); return TRACS_E_ARG; }
    if (a->L) {
        DeviceArray<unsigned> d_counts;
        int rc = d_counts.alloc(n, "sample counts");
        if (rc || (rc = sample_n_counts(a, rule->keep, rule->keep_len, d_counts.get(), nullptr))) return rc;
        TRACS_HIP_CHECK(hipMemcpy(src.n_count.data(), d_counts.get(), n * 4, hipMemcpyDeviceToHost));
    }
    const double limit = std::floor(rule->max_sample_share * (double)src.rule_sites);
    size_t kept0 = 0, kept1 = 0;
    for (size_t s = 0; s < n; s++) {
        src.kept[s] = (double)src.n_count[s] <= limit;
        if (src.kept[s]) (s < *n0 ? kept0 : kept1)++;
    }
    if (kept0 + kept1 == 0 || (n_fasta == 2 && (kept0 == 0 || kept1 == 0))) { set_error("no sample left after the sample rule"); return TRACS_E_ARG; }
    if (kept0 + kept1 == n) return TRACS_OK;
    tracs_alignment *sel = nullptr;
    const int rc = select_samples(a, src.kept.data(), &sel, nullptr, true);
    if (rc) return rc;
    tracs_alignment_free(a);
    *pa = sel;
    std::vector<std::string> names;
    names.reserve(kept0 + kept1);
    for (size_t s = 0; s < n; s++)
        if (src.kept[s]) names.push_back(std::move(fd.names[s]));
    fd.names = std::move(names);
    fd.n = kept0 + kept1;
    if (n_fasta == 2) *n0 = kept0;
    else *n0 = fd.n;
    return TRACS_OK;
}

static int pairsnp_run(const char *const *fasta, int n_fasta, int dist, int filter, SiteRule *rule, tracs_pairsnp_result **out);
static int nearest_run(const char *const *fasta, int n_fasta, int k, int dist, int filter, SiteRule *rule, tracs_pairsnp_result **out);

int tracs_pairsnp(const char *const *fasta, int n_fasta, int n_threads, int dist, int filter, tracs_pairsnp_result **out)
{
    (void)n_threads;
    return pairsnp_run(fasta, n_fasta, dist, filter, nullptr, out);
}

int tracs_pairsnp_sites(const char *const *fasta, int n_fasta, int n_threads, int dist, int filter, const uint64_t *keep, size_t keep_len,
                        uint32_t max_n_samples, tracs_pairsnp_result **out)
{
    (void)n_threads;
    SiteRule rule;
    rule.keep = keep; rule.keep_len = keep_len; rule.max_n = max_n_samples;
    return pairsnp_run(fasta, n_fasta, dist, filter, rule.active() ? &rule : nullptr, out);
}

int tracs_nearest_sites(const char *const *fasta, int n_fasta, int n_threads, int k, int dist, int filter, const uint64_t *keep,
                        size_t keep_len, uint32_t max_n_samples, tracs_pairsnp_result **out)
{
    (void)n_threads;
    SiteRule rule;
    rule.keep = keep; rule.keep_len = keep_len; rule.max_n = max_n_samples;
    return nearest_run(fasta, n_fasta, k, dist, filter, rule.active() ? &rule : nullptr, out);
}

// a tracs_rules of the _rules entry points -> the rule the runs take; a share outside [0, 1] (a NaN too) and both forms of the N rule
// at once are refused.  No field set at all: no rule, call for call the plain entry points.
static int rules_from_struct(const tracs_rules *in, SiteRule &rule, bool *any)
{
    *any = false;
    if (!in) return TRACS_OK;
    for (double share : {in->max_n_share, in->max_sample_n_share})
        if (!(share < 0.0) && !(share <= 1.0)) { set_error("tracs_rules: a share must be in [0, 1], or negative for no rule"); return TRACS_E_ARG; }
    if (!(in->max_n_share < 0.0) && in->max_n_samples != UINT32_MAX) {
        set_error("tracs_rules: max_n_share and max_n_samples are two forms of one rule; give one");
        return TRACS_E_ARG;
    }
    rule.keep = in->keep; rule.keep_len = in->keep_len; rule.max_n = in->max_n_samples;
    if (!(in->max_n_share < 0.0)) rule.max_n_share = in->max_n_share;
    if (!(in->max_sample_n_share < 0.0)) rule.max_sample_share = in->max_sample_n_share;
    rule.min_sites = in->min_sites;
    *any = rule.active() || rule.max_n_share >= 0.0 || rule.sample_rule() || rule.min_sites != 0;
    return TRACS_OK;
}

int tracs_pairsnp_rules(const char *const *fasta, int n_fasta, int n_threads, int dist, int filter, const tracs_rules *rules,
                        tracs_pairsnp_result **out)
{
    (void)n_threads;
    SiteRule rule;
    bool any = false;
    if (out) *out = nullptr;
    const int rc = rules_from_struct(rules, rule, &any);
    if (rc) return rc;
    return pairsnp_run(fasta, n_fasta, dist, filter, any ? &rule : nullptr, out);
}

int tracs_nearest_rules(const char *const *fasta, int n_fasta, int n_threads, int k, int dist, int filter, const tracs_rules *rules,
                        tracs_pairsnp_result **out)
{
    (void)n_threads;
    SiteRule rule;
    bool any = false;
    if (out) *out = nullptr;
    const int rc = rules_from_struct(rules, rule, &any);
    if (rc) return rc;
    return nearest_run(fasta, n_fasta, k, dist, filter, any ? &rule : nullptr, out);
}

// read + pack for the array entry points: the alignment and the result that will carry its pairs, both owned
static int result_from_fasta(const char *const *fasta, int n_fasta, SiteRule *rule, AlignmentOwner &a, ResultOwner &res,
                             size_t *n0)
{
    tracs_alignment *packed = nullptr;
    char *names = nullptr;
    size_t names_bytes = 0;
    const int rc = alignment_from_fasta_sites(fasta, n_fasta, &packed, &names, &names_bytes, n0, rule);
    if (rc) return rc;
    a.reset(packed);
    res.reset(new tracs_pairsnp_result());
    res->nseq = a->n; res->L = a->L;
    if (rule) res->source = std::move(rule->source);
    else res->source.rule_sites = a->L;
    { size_t o = 0; for (size_t i = 0; i < a->n; i++) { res->names.emplace_back(names + o); o += res->names.back().size() + 1; } }
    tracs_free(names);
    return TRACS_OK;
}

static int pairsnp_run(const char *const *fasta, int n_fasta, int dist, int filter, SiteRule *rule, tracs_pairsnp_result **out)
{
    if (!out) { set_error("tracs_pairsnp: out is NULL"); return TRACS_E_ARG; }
    *out = nullptr;
    if (n_fasta < 1 || n_fasta > 2 || !fasta) { set_error("Invalid number of fasta files!"); return TRACS_E_ARG; }   // :340-343
    SigintScope sigint;
    AlignmentOwner a;
    ResultOwner res;
    size_t n0 = 0;
    int rc = result_from_fasta(fasta, n_fasta, rule, a, res, &n0);
    if (rc) return rc;
    StageClock clock;
    double t_dense = 0.0, t_coo = 0.0, t_pull = 0.0, t_filter = 0.0;
    PanelWalk walk(a.get(), n_fasta, n0, dist, rule ? rule->min_sites : 0,
                   [&](Lap l) { lap(clock, l == LAP_DENSE ? t_dense : l == LAP_COO ? t_coo : t_filter); });
    PairStage stage(walk, filter);
    if (walk.any()) {
        if ((rc = walk.begin(true, false))) return rc;
        std::vector<unsigned> h32;
        PairColumns c;
        for (Panel pn; walk.more();) {
            lap(clock, t_pull);
            if ((rc = walk.next(pn)) || (rc = stage.extract(pn, c))) return rc;
            if (!c.total) continue;
            h32.resize(c.total);
            auto pull = [&](const unsigned *src, std::vector<uint64_t> &dst) -> int {
                TRACS_HIP_CHECK(hipMemcpy(h32.data(), src, c.total * 4, hipMemcpyDeviceToHost));
                widen_append(dst, h32.data(), c.total);
                return TRACS_OK;
            };
            if ((rc = pull(c.rows, res->rows)) || (rc = pull(c.cols, res->cols)) || (rc = pull(c.d, res->dist)) || (rc = pull(c.nn, res->ncomp))) return rc;
            if (filter && (rc = pull(c.filt, res->filt))) return rc;
            lap(clock, t_pull);
        }
    }
    if (clock.on)
        std::fprintf(stderr, "[stage] dense panels (once-per-pack work + pair kernels) %.4f s\n[stage] COO extraction (device) %.4f s\n"
                             "[stage] COO D2H + widening to uint64 (%zu pairs) %.4f s\n[stage] recombination filter %.4f s\n",
                     t_dense, t_coo, res->rows.size(), t_pull, t_filter);
    // a Ctrl-C that arrived during the last panel / filter batch is not swallowed (the reference looks at its flag on every row)
    if (g_sigint) return interrupted();
    if (!filter) res->filt.assign(res->rows.size(), 0);      // filter off: `len` zeros (:452 via combine_vectors :31)
    *out = res.release();
    return TRACS_OK;
}

// (min, max) of each emitted pair: the recombination filter's pairs are (i, j > i), as tracs_pairsnp emits them
__global__ __launch_bounds__(256) void knn_pair_order_kernel(const unsigned *__restrict__ rows, const unsigned *__restrict__ cols, size_t n,
                                                             unsigned *__restrict__ lo, unsigned *__restrict__ hi)
{
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (size_t)gridDim.x * 256) {
        const unsigned r = rows[t], c = cols[t];
        lo[t] = r < c ? r : c;
        hi[t] = r < c ? c : r;
    }
}

// k nearest neighbours per sample (include/tracs_hip.h): FASTA -> planes -> row panels of tracs_pairsnp_dense_thr ->
// tracs_knn_update -> tracs_knn_emit -> (filter) tracs_filter_recomb_pairs on the emitted pairs -> one device-to-host copy.
int tracs_nearest(const char *const *fasta, int n_fasta, int n_threads, int k, int dist, int filter, tracs_pairsnp_result **out)
{
    (void)n_threads;
    return nearest_run(fasta, n_fasta, k, dist, filter, nullptr, out);
}

static int nearest_run(const char *const *fasta, int n_fasta, int k, int dist, int filter, SiteRule *rule, tracs_pairsnp_result **out)
{
    if (!out) { set_error("tracs_nearest: out is NULL"); return TRACS_E_ARG; }
    *out = nullptr;
    if (n_fasta < 1 || n_fasta > 2 || !fasta) { set_error("Invalid number of fasta files!"); return TRACS_E_ARG; }
    if (k < 1 || k > 1024) { set_error("tracs_nearest: k must be in [1, 1024]"); return TRACS_E_ARG; }
    SigintScope sigint;
    AlignmentOwner a;
    ResultOwner res;
    size_t n0 = 0;
    int rc = result_from_fasta(fasta, n_fasta, rule, a, res, &n0);
    if (rc) return rc;
    const size_t n = a->n;
    const size_t n_lists = n_fasta == 1 ? n : n0;                   // two files: lists for the samples of file 0 only
    PanelWalk walk(a.get(), n_fasta, n0, dist, rule ? rule->min_sites : 0);
    DeviceBuffer d_state, d_off, d_out;
    StageClock clock;
    if (walk.any()) {
        if ((rc = d_state.alloc(tracs_knn_state_bytes(n_lists, k), "state")) || (rc = tracs_knn_init(d_state.ptr, n_lists, k, nullptr))) return rc;
        if ((rc = walk.begin(false, false))) return rc;
        for (Panel pn; walk.more();) {
            if ((rc = walk.next(pn))) return rc;
            if ((rc = tracs_knn_update(pn.bd, pn.bn, n, n, pn.r0, pn.r1, walk.j_start, dist, k, n_fasta == 1 ? 1 : 0, d_state.ptr, nullptr))) return rc;
        }
        clock.mark("dense panels + selection");
        // rows, cols, d, nn, filt (and the filter's ordered pairs) in one block: one copy back
        const size_t cap = n_lists * (size_t)k;
        if ((rc = d_off.alloc((n_lists + 1) * 8, "off")) || (rc = d_out.alloc(cap * 4 * (filter ? 7 : 4), "out"))) return rc;
        unsigned *c_rows = d_out.as<unsigned>(), *c_cols = c_rows + cap, *c_d = c_rows + 2 * cap, *c_n = c_rows + 3 * cap;
        if ((rc = tracs_knn_emit(d_state.ptr, 0, n_lists, k, d_off.as<int64_t>(), c_rows, c_cols, c_d, c_n, nullptr))) return rc;
        long long tot = 0;
        TRACS_HIP_CHECK(hipMemcpy(&tot, d_off.as<int64_t>() + n_lists, 8, hipMemcpyDeviceToHost));
        const size_t total = (size_t)tot;
        clock.mark("emit");
        if (filter && total) {
            if (g_sigint) return interrupted();
            unsigned *c_f = c_rows + 4 * cap, *c_lo = c_rows + 5 * cap, *c_hi = c_rows + 6 * cap;
            hipLaunchKernelGGL(knn_pair_order_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 65535)), dim3(256), 0, nullptr,
                               c_rows, c_cols, total, c_lo, c_hi);
            TRACS_HIP_CHECK(hipGetLastError());
            if ((rc = tracs_filter_recomb_pairs(a.get(), c_lo, c_hi, c_d, total, c_f, nullptr))) return rc;
            clock.mark("recombination filter");
        }
        if (total) {
            const size_t ncol = filter ? 5 : 4;
            std::vector<unsigned> h32(ncol * total);
            TRACS_HIP_CHECK(hipMemcpy2D(h32.data(), total * 4, c_rows, cap * 4, total * 4, ncol, hipMemcpyDeviceToHost));
            widen_append(res->rows, h32.data(), total);
            widen_append(res->cols, h32.data() + total, total);
            widen_append(res->dist, h32.data() + 2 * total, total);
            widen_append(res->ncomp, h32.data() + 3 * total, total);
            if (filter) widen_append(res->filt, h32.data() + 4 * total, total);
            clock.mark("D2H + widening");
        }
    }
    if (g_sigint) return interrupted();
    if (!filter) res->filt.assign(res->rows.size(), 0);
    *out = res.release();
    return TRACS_OK;
}

// ---- `tracs distance` for one alignment, results on the device until the CSV rows (tracs/distance.py:159-258) --------------------------
// open: read + pack the FASTA(s) (the names are what the caller needs to look the sampling dates up); run: row panel by row panel --
// dense call (d, compared sites; early out beyond the threshold), transcluster on the panel (P(direct), E(K): src/transcluster.hpp:
// 240-287 through the dense route, delta from the day numbers), the pairs within the threshold extracted in row-major order
// (src/pairsnp.hpp:451-455) with their P and E(K) -- then ONE device-to-host pass, a few million rows at a time, each batch formatted
// and written by the host threads while the next one arrives.  Nothing widens to uint64, nothing goes back to the device.
struct tracs_distance {
    tracs_alignment *a = nullptr;
    std::vector<std::string> names;
    std::vector<const char *> name_ptr;
    size_t n0 = 0;
    int n_fasta = 0;
    size_t source_len = 0;               // columns read (site rules: h->a holds the kept ones)
    std::vector<uint64_t> kept;          // the kept columns; empty: every column
    uint32_t min_sites = 0;              // the pair rule of _run, _forest and _histogram (0: none)
    SourceSamples source;                // the records read (sample rule: h->a and names hold the survivors)
};

static int distance_open(const char *const *fasta, int n_fasta, SiteRule *rule, tracs_distance **out)
{
    if (!out) { set_error("tracs_distance_open: out is NULL"); return TRACS_E_ARG; }
    *out = nullptr;
    if (n_fasta < 1 || n_fasta > 2 || !fasta) { set_error("Invalid number of fasta files!"); return TRACS_E_ARG; }   // :340-343
    auto *h = new tracs_distance();
    char *names = nullptr;
    size_t names_bytes = 0;
    const int rc = alignment_from_fasta_sites(fasta, n_fasta, &h->a, &names, &names_bytes, &h->n0, rule);
    if (rc) { delete h; return rc; }
    h->source_len = rule ? rule->source_len : h->a->L;
    if (rule) { h->kept = std::move(rule->kept); h->min_sites = rule->min_sites; h->source = std::move(rule->source); }
    else h->source.rule_sites = h->a->L;
    h->n_fasta = n_fasta;
    { size_t o = 0; for (size_t i = 0; i < h->a->n; i++) { h->names.emplace_back(names + o); o += h->names.back().size() + 1; } }
    tracs_free(names);
    for (auto &s : h->names) h->name_ptr.push_back(s.c_str());
    *out = h;
    return TRACS_OK;
}

int tracs_distance_open(const char *const *fasta, int n_fasta, tracs_distance **out) { return distance_open(fasta, n_fasta, nullptr, out); }

int tracs_distance_open_sites(const char *const *fasta, int n_fasta, const uint64_t *keep, size_t keep_len, uint32_t max_n_samples,
                              tracs_distance **out)
{
    SiteRule rule;
    rule.keep = keep; rule.keep_len = keep_len; rule.max_n = max_n_samples;
    return distance_open(fasta, n_fasta, rule.active() ? &rule : nullptr, out);
}

int tracs_distance_open_rules(const char *const *fasta, int n_fasta, const tracs_rules *rules, tracs_distance **out)
{
    SiteRule rule;
    bool any = false;
    if (out) *out = nullptr;
    const int rc = rules_from_struct(rules, rule, &any);
    if (rc) return rc;
    return distance_open(fasta, n_fasta, any ? &rule : nullptr, out);
}

// the records read, before the sample rule (without one: the loaded samples, all kept, counts 0)
static size_t source_nseq(const SourceSamples &s, const std::vector<std::string> &names) { return s.names.empty() ? names.size() : s.names.size(); }
static const char *source_name(const SourceSamples &s, const std::vector<std::string> &names, size_t i)
{
    const std::vector<std::string> &v = s.names.empty() ? names : s.names;
    return i < v.size() ? v[i].c_str() : nullptr;
}
static uint32_t source_n_count(const SourceSamples &s, size_t i) { return i < s.n_count.size() ? s.n_count[i] : 0; }
static int source_kept(const SourceSamples &s, const std::vector<std::string> &names, size_t i)
{
    return s.names.empty() ? (i < names.size() ? 1 : 0) : (i < s.kept.size() ? (int)s.kept[i] : 0);
}

size_t tracs_distance_source_nseq(const tracs_distance *h) { return h ? source_nseq(h->source, h->names) : 0; }
const char *tracs_distance_source_name(const tracs_distance *h, size_t i) { return h ? source_name(h->source, h->names, i) : nullptr; }
uint32_t tracs_distance_source_n_count(const tracs_distance *h, size_t i) { return h ? source_n_count(h->source, i) : 0; }
int tracs_distance_source_kept(const tracs_distance *h, size_t i) { return h ? source_kept(h->source, h->names, i) : 0; }
size_t tracs_distance_rule_sites(const tracs_distance *h) { return h ? h->source.rule_sites : 0; }
size_t tracs_pairsnp_source_nseq(const tracs_pairsnp_result *r) { return r ? source_nseq(r->source, r->names) : 0; }
const char *tracs_pairsnp_source_name(const tracs_pairsnp_result *r, size_t i) { return r ? source_name(r->source, r->names, i) : nullptr; }
uint32_t tracs_pairsnp_source_n_count(const tracs_pairsnp_result *r, size_t i) { return r ? source_n_count(r->source, i) : 0; }
int tracs_pairsnp_source_kept(const tracs_pairsnp_result *r, size_t i) { return r ? source_kept(r->source, r->names, i) : 0; }
size_t tracs_pairsnp_rule_sites(const tracs_pairsnp_result *r) { return r ? r->source.rule_sites : 0; }

size_t tracs_distance_source_len(const tracs_distance *h) { return h ? h->source_len : 0; }
size_t tracs_distance_len(const tracs_distance *h) { return (h && h->a) ? h->a->L : 0; }
int tracs_distance_kept_sites(const tracs_distance *h, uint64_t *kept)
{
    if (!h || !kept) { set_error("tracs_distance_kept_sites: NULL argument"); return TRACS_E_ARG; }
    const size_t words = (h->source_len + 63) / 64;
    if (!h->kept.empty()) { std::memcpy(kept, h->kept.data(), words * 8); return TRACS_OK; }
    for (size_t w = 0; w < words; w++) kept[w] = ~0ull;
    if (h->source_len & 63) kept[words - 1] = (1ull << (h->source_len & 63)) - 1;
    return TRACS_OK;
}

size_t tracs_distance_nseq(const tracs_distance *h) { return h ? h->names.size() : 0; }
const char *tracs_distance_name(const tracs_distance *h, size_t i) { return (h && i < h->names.size()) ? h->names[i].c_str() : nullptr; }
void tracs_distance_free(tracs_distance *h) { if (h) { if (h->a) tracs_alignment_free(h->a); delete h; } }

// ---- what the handle compares, looked at and written out (csrc/msa_out.hip) -----------------------------------------
int tracs_distance_site_census(tracs_distance *h, uint32_t *counts_host, uint64_t *differs_host, size_t *n_differs)
{
    if (n_differs) *n_differs = 0;
    if (!h || !h->a) { set_error("tracs_distance_site_census: NULL argument"); return TRACS_E_ARG; }
    const tracs_alignment *a = h->a;
    if (!a->L) return TRACS_OK;
    DeviceArray<uint32_t> d_counts;
    int rc = counts_host ? d_counts.alloc(a->L * 6, "site census") : TRACS_OK;
    if (rc || (rc = site_census(a, d_counts.get(), differs_host, n_differs, nullptr))) return rc;
    if (counts_host) TRACS_HIP_CHECK(hipMemcpy(counts_host, d_counts.get(), a->L * 6 * 4, hipMemcpyDeviceToHost));
    return TRACS_OK;
}

// Batches of samples: device buffer -> pinned host buffer -> writer.  The two buffers hold `batch` rows of `stride` bytes (the row
// length rounded up to 16, so every row takes the kernel's 16-byte stores): at most 256 MiB each, or one row when a row is longer --
// whatever n is.  The writer adds one compressed member per thread.
int tracs_distance_write_alignment(tracs_distance *h, const char *path, size_t sample_begin, size_t sample_end, int differing_only,
                                   int n_threads, int gzip_level, size_t *sites_written)
{
    if (sites_written) *sites_written = 0;
    if (!h || !h->a || !path) { set_error("tracs_distance_write_alignment: NULL argument"); return TRACS_E_ARG; }
    if (sample_begin > sample_end || sample_end > h->a->n) { set_error("tracs_distance_write_alignment: sample range outside the alignment"); return TRACS_E_ARG; }
    const tracs_alignment *a = h->a;
    AlignmentOwner cut;
    int rc = TRACS_OK;
    if (differing_only) {
        std::vector<uint64_t> differs((a->L + 63) / 64, 0);
        size_t nd = 0;
        tracs_alignment *sel = nullptr;
        if ((rc = site_census(a, nullptr, differs.data(), &nd, nullptr))) return rc;
        if (!nd) { set_error("no column differs among the samples"); return TRACS_E_ARG; }
        if ((rc = select_sites(const_cast<tracs_alignment *>(a), differs.data(), a->L, UINT32_MAX, &sel, nullptr, nullptr, nullptr, false))) return rc;
        cut.reset(sel);
        a = sel;
    }
    const size_t L = a->L, stride = (L + 15) / 16 * 16, count = sample_end - sample_begin;
    const size_t batch = std::max<size_t>(1, std::min<size_t>(count, stride ? (256ull << 20) / stride : count));
    DeviceBuffer d_buf;
    PinnedBuffer h_buf;
    if (count && L && ((rc = d_buf.alloc(batch * stride, "buf")) || (rc = h_buf.alloc(batch * stride, "buf")))) return rc;
    if ((rc = tracs_write_fasta_rows(path, nullptr, nullptr, stride, 0, L, 0, n_threads, gzip_level))) return rc;     // truncate
    for (size_t s = sample_begin; s < sample_end; s += batch) {
        const size_t cnt = std::min(batch, sample_end - s);
        if (L) {
            if ((rc = unpack_rows(a, s, cnt, d_buf.as<uint8_t>(), stride, nullptr))) return rc;
            TRACS_HIP_CHECK(hipMemcpy(h_buf.ptr, d_buf.ptr, cnt * stride, hipMemcpyDeviceToHost));
        }
        if ((rc = tracs_write_fasta_rows(path, h->name_ptr.data() + s, h_buf.as<uint8_t>(), stride, cnt, L, 1, n_threads, gzip_level))) return rc;
    }
    if (sites_written) *sites_written = L;
    return TRACS_OK;
}

// ---- the sites behind listed pairs (csrc/pair_sites.hip) --------------------------------------------------------------
tracs_alignment *tracs_distance_alignment(tracs_distance *h) { return h ? h->a : nullptr; }

int tracs_distance_pair_sites(tracs_distance *h, const uint32_t *rows, const uint32_t *cols, size_t n_pairs, int filter, uint64_t max_entries,
                              const char *path, const char *const *contig_names, const uint64_t *contig_lengths, size_t n_contigs,
                              int n_threads, uint64_t *rows_written)
{
    if (rows_written) *rows_written = 0;
    if (!h || !h->a) { set_error("tracs_distance_pair_sites: NULL argument"); return TRACS_E_ARG; }
    return pair_sites_write(h->a, h->name_ptr.data(), h->kept.empty() ? nullptr : h->kept.data(), h->source_len, rows, cols, n_pairs, filter,
                            max_entries, path, contig_names, contig_lengths, n_contigs, n_threads, rows_written);
}

int tracs_distance_run(tracs_distance *h, int dist, const int32_t *days, double lamb, double beta, double precision, double k_max,
                       const char *path, const char *ref, int filter, uint64_t *rows_written, uint64_t *n_pairs)
{
    if (rows_written) *rows_written = 0;
    if (n_pairs) *n_pairs = 0;
    if (!h || !h->a || !path || !ref) { set_error("tracs_distance_run: NULL argument"); return TRACS_E_ARG; }
    SigintScope sigint;
    const bool with_dates = days != nullptr;
    // rows per device-to-host batch (TRACS_DISTANCE_BATCH_ROWS: diagnostics -- small batches in tests)
    const long long env_rows = sw::integer(sw::TRACS_DISTANCE_BATCH_ROWS, 0LL);
    const size_t batch_rows = env_rows >= 16 ? (size_t)env_rows : 0;            // (below 16: as if not set)
    // (never more than the pairs there can be: ten isolates do not pin a quarter of a gigabyte of host memory)
    const size_t CH = std::max<size_t>(64, std::min<size_t>(batch_rows ? batch_rows : (size_t)1 << 22, (h->n_fasta == 1 ? h->a->n : h->n0) * h->a->n));
    tracs::DistanceRowWriter writer;
    int rc = writer.open(path, h->name_ptr.data(), h->name_ptr.size(), ref);
    if (rc) return rc;
    StageClock clock;
    double t_dense = 0.0, t_tc = 0.0, t_coo = 0.0, t_rows = 0.0;
    // (the extraction's own lap stays with the sum that follows it, as the table of DESIGN.md 5 has it)
    PanelWalk walk(h->a, h->n_fasta, h->n0, dist, h->min_sites, [&](Lap l) { if (l != LAP_COO) lap(clock, l == LAP_DENSE ? t_dense : t_tc); });
    // --filter: the transmission model is driven by the FILTERED distance (tracs/distance.py:183-193): per emitted pair, after the filter
    PairStage stage(walk, filter, lamb, beta, precision);
    PinnedBuffer pin[2];
    CopyLane lane;                                                  // (after `pin`: drained and destroyed before they are freed)
    uint64_t pairs = 0;
    if (walk.any()) {
        if (with_dates && (rc = stage.set_days(days))) return rc;
        if ((rc = walk.begin(true, stage.dense_tc()))) return rc;
        // a batch on the host: four uint32 columns (five with --filter), then two f64 ones; two of them, so that one is formatted while the
        // next arrives
        const size_t n32 = filter ? 5 : 4;
        const size_t batch_bytes = CH * (n32 * 4 + (with_dates ? 16 : 0) + 4);
        const size_t f64_at = (CH * n32 * 4 + 7) / 8 * 8;
        for (auto &q : pin) if ((rc = q.alloc(batch_bytes, "row batch"))) return rc;
        if ((rc = lane.create())) return rc;
        std::vector<uint32_t> zeros;                                  // the filtered column without metadata: `len` zeros (:240-258)
        if (!with_dates) zeros.assign(CH, 0u);
        PairColumns c;
        for (Panel pn; walk.more();) {
            if ((rc = walk.next(pn)) || (rc = stage.extract(pn, c))) return rc;
            if (!c.total) continue;
            TRACS_HIP_CHECK(hipEventRecord(lane.ready, nullptr));
            TRACS_HIP_CHECK(hipStreamWaitEvent(lane.stream, lane.ready, 0));
            lap(clock, t_coo);
            const size_t nb = (c.total + CH - 1) / CH;
            auto post = [&](size_t k) -> hipError_t {                 // batch k -> pinned set k % 2
                const size_t o = k * CH, cnt = std::min(CH, c.total - o);
                char *dst = pin[k & 1].as<char>();
                const unsigned *src32[5] = {c.rows, c.cols, c.d, c.nn, c.filt};
                for (size_t q = 0; q < n32; q++) {
                    const hipError_t e = hipMemcpyAsync(dst + (size_t)q * CH * 4, src32[q] + o, cnt * 4, hipMemcpyDeviceToHost, lane.stream);
                    if (e != hipSuccess) return e;
                }
                if (with_dates) {
                    hipError_t e = hipMemcpyAsync(dst + f64_at, c.p + o, cnt * 8, hipMemcpyDeviceToHost, lane.stream);
                    if (e == hipSuccess) e = hipMemcpyAsync(dst + f64_at + CH * 8, c.e + o, cnt * 8, hipMemcpyDeviceToHost, lane.stream);
                    if (e != hipSuccess) return e;
                }
                return hipEventRecord(lane.ev[k & 1], lane.stream);
            };
            TRACS_HIP_CHECK(post(0));
            for (size_t k = 0; k < nb; k++) {
                if (g_sigint) { (void)hipStreamSynchronize(lane.stream); return interrupted(); }
                TRACS_HIP_CHECK(hipEventSynchronize(lane.ev[k & 1]));
                if (k + 1 < nb) TRACS_HIP_CHECK(post(k + 1));
                const size_t cnt = std::min(CH, c.total - k * CH);
                const char *src = pin[k & 1].as<char>();
                const uint32_t *hr = reinterpret_cast<const uint32_t *>(src), *hc = hr + CH, *hd = hr + 2 * CH, *hn = hr + 3 * CH;
                const double *hp = reinterpret_cast<const double *>(src + f64_at), *he = hp + CH;
                // the filtered column: --filter: the filtered distances; else metadata on: a column of "NA" (:204), metadata off: zeros (:240-258)
                const uint32_t *hf = filter ? hr + 4 * CH : (with_dates ? nullptr : zeros.data());
                if ((rc = writer.append_u32(hr, hc, hd, hf, hn, days, with_dates ? hp : nullptr, with_dates ? he : nullptr,
                                            cnt, with_dates ? 1 : 0, with_dates ? k_max : -1.0))) return rc;
            }
            pairs += (uint64_t)c.total;
            lap(clock, t_rows);
        }
    }
    if (clock.on)
        std::fprintf(stderr, "[stage] dense panels (once-per-pack work + pair kernels) %.4f s\n[stage] transcluster on the panels (device) %.4f s\n"
                             "[stage] COO extraction (device) %.4f s\n[stage] rows: device -> host, format, write (%llu pairs) %.4f s\n",
                     t_dense, t_tc, t_coo, (unsigned long long)pairs, t_rows);
    rc = writer.close();
    if (rows_written) *rows_written = writer.written();
    if (n_pairs) *n_pairs = pairs;
    if (g_sigint) return interrupted();
    return rc;
}

// The rows that --mst and --ancestors keep, `count` < n of them: rows, cols, d, nn, filt (uint32), P, E(K) (f64) emitted into fresh
// columns, copied to the host and written through the row writer.  The filtered column as the full run writes it: --filter: the
// filtered distances; else metadata on: "NA" (:204), metadata off: the emitted column (zeros, :240-258).
using EmitFn = std::function<int(unsigned *, unsigned *, unsigned *, unsigned *, unsigned *, double *, double *)>;
static int write_emitted_rows(size_t count, const EmitFn &emit, tracs::DistanceRowWriter &writer, const int32_t *days, int filter)
{
    DeviceBuffer coo, cp;
    int rc;
    if ((rc = coo.alloc(count * 4 * 5, "coo")) || (rc = cp.alloc(count * 16, "cp"))) return rc;
    unsigned *c = coo.as<unsigned>();
    double *f = cp.as<double>();
    if ((rc = emit(c, c + count, c + 2 * count, c + 3 * count, c + 4 * count, f, f + count))) return rc;
    std::vector<uint32_t> h32(count * 5);
    std::vector<double> h64(count * 2);
    TRACS_HIP_CHECK(hipMemcpy(h32.data(), c, count * 20, hipMemcpyDeviceToHost));
    TRACS_HIP_CHECK(hipMemcpy(h64.data(), f, count * 16, hipMemcpyDeviceToHost));
    const uint32_t *hr = h32.data(), *hc = hr + count, *hd = hr + 2 * count, *hn = hr + 3 * count, *hf = hr + 4 * count;
    const bool with_dates = days != nullptr;
    return writer.append_u32(hr, hc, hd, (filter || !with_dates) ? hf : nullptr, hn, days, with_dates ? h64.data() : nullptr,
                             with_dates ? h64.data() + count : nullptr, count, with_dates ? 1 : 0, -1.0);
}

// the column a pair is weighed by: 0 d, 1 filtered d, 2 P(direct), 3 E(K) (the columns `cluster -D` reads: 3, 6, 4, 5)
static const void *weight_column(const PairColumns &c, int weight)
{
    return weight == 0 ? (const void *)c.d : weight == 1 ? (const void *)c.filt : weight == 2 ? (const void *)c.p : (const void *)c.e;
}

// `tracs distance --mst WEIGHT` for one alignment (include/tracs_hip.h): the panel walk and the pair stage of
// tracs_distance_run (the panel's pairs within the threshold with P and E(K), --filter's filtered distances and their P and E(K)),
// then tracs_msf_update_coo instead of the rows; after the last panel the forest is emitted and written through the same row writer.
int tracs_distance_forest(tracs_distance *h, int dist, const int32_t *days, double lamb, double beta, double precision, double k_max,
                          int filter, int weight, const char *path, const char *ref, uint64_t *rows_written, uint64_t *n_eligible)
{
    if (rows_written) *rows_written = 0;
    if (n_eligible) *n_eligible = 0;
    if (!h || !h->a || !path || !ref) { set_error("tracs_distance_forest: NULL argument"); return TRACS_E_ARG; }
    if (weight < 0 || weight > 3) { set_error("tracs_distance_forest: weight must be 0 (snp), 1 (filter), 2 (direct) or 3 (expectedK)"); return TRACS_E_ARG; }
    if (weight == 1 && !filter) { set_error("tracs_distance_forest: the filter weight needs filter != 0"); return TRACS_E_ARG; }
    if (weight >= 2 && !days) { set_error("tracs_distance_forest: the direct and expectedK weights need sampling dates"); return TRACS_E_ARG; }
    SigintScope sigint;
    const size_t n = h->a->n;
    tracs::DistanceRowWriter writer;
    int rc = writer.open(path, h->name_ptr.data(), h->name_ptr.size(), ref);
    if (rc) return rc;
    StageClock clock;
    uint64_t eligible = 0;
    const double e_max = (days && k_max >= 0.0) ? k_max : -1.0;
    PanelWalk walk(h->a, h->n_fasta, h->n0, dist, h->min_sites);
    PairStage stage(walk, filter, lamb, beta, precision);
    DeviceBuffer d_state;
    if (walk.any()) {
        if ((rc = d_state.alloc(tracs_msf_state_bytes(n), "state")) || (rc = tracs_msf_init(d_state.ptr, n, nullptr))) return rc;
        if (days && (rc = stage.set_days(days))) return rc;
        if ((rc = walk.begin(true, stage.dense_tc()))) return rc;
        PairColumns c;
        for (Panel pn; walk.more();) {
            if ((rc = walk.next(pn)) || (rc = stage.extract(pn, c))) return rc;
            if (!c.total) continue;
            // -K drops pairs with E(K) above it or NaN
            uint64_t taken = 0;
            if ((rc = tracs_msf_update_coo(d_state.ptr, n, c.total, c.rows, c.cols, weight_column(c, weight), weight >= 2 ? 1 : 0,
                                           e_max >= 0.0 ? c.e : nullptr, e_max, c.d, c.nn, c.filt, c.p, c.e, &taken, nullptr))) return rc;
            eligible += taken;
        }
        clock.mark("dense panels + transcluster + forest updates");
        size_t nf = 0;
        if ((rc = tracs_msf_emit(d_state.ptr, n, &nf, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))) return rc;
        stage.release();
        if (nf && (rc = write_emitted_rows(nf, [&](unsigned *r, unsigned *cc, unsigned *d, unsigned *nn, unsigned *f, double *p, double *e) {
                       return tracs_msf_emit(d_state.ptr, n, &nf, r, cc, d, nn, f, p, e, nullptr); }, writer, days, filter))) return rc;
        clock.mark("forest rows: emit, device -> host, format, write");
    }
    rc = writer.close();
    if (rows_written) *rows_written = writer.written();
    if (n_eligible) *n_eligible = eligible;
    if (g_sigint) return interrupted();
    return rc;
}

// `tracs distance --ancestors WEIGHT` for one alignment (include/tracs_hip.h): as tracs_distance_forest, with
// tracs_anc_update_coo instead of the forest update; after the last panel the links are emitted and written through the same row
// writer, and the tree file is written from parent / root / generation.
int tracs_distance_ancestors(tracs_distance *h, int dist, const int32_t *days, double lamb, double beta, double precision, double k_max,
                             int filter, int weight, const char *path, const char *ref, const char *tree_path,
                             const char *const *meta_dates, uint64_t *rows_written, uint64_t *n_eligible)
{
    if (rows_written) *rows_written = 0;
    if (n_eligible) *n_eligible = 0;
    if (!h || !h->a || !path || !ref) { set_error("tracs_distance_ancestors: NULL argument"); return TRACS_E_ARG; }
    if (weight < 0 || weight > 3) { set_error("tracs_distance_ancestors: weight must be 0 (snp), 1 (filter), 2 (direct) or 3 (expectedK)"); return TRACS_E_ARG; }
    if (weight == 1 && !filter) { set_error("tracs_distance_ancestors: the filter weight needs filter != 0"); return TRACS_E_ARG; }
    if (!days) { set_error("tracs_distance_ancestors: sampling dates are required (they order the samples)"); return TRACS_E_ARG; }
    if (tree_path && !meta_dates) { set_error("tracs_distance_ancestors: the tree file needs the samples' dates as text"); return TRACS_E_ARG; }
    SigintScope sigint;
    const size_t n = h->a->n;
    tracs::DistanceRowWriter writer;
    int rc = writer.open(path, h->name_ptr.data(), h->name_ptr.size(), ref);
    if (rc) return rc;
    StageClock clock;
    uint64_t eligible = 0;
    const double e_max = k_max >= 0.0 ? k_max : -1.0;
    std::vector<uint32_t> tree(n * 3);                              // parent, root, generation
    for (size_t s = 0; s < n; s++) { tree[s] = 0xFFFFFFFFu; tree[n + s] = (uint32_t)s; tree[2 * n + s] = 0; }      // (no pair at all: every sample a root)
    PanelWalk walk(h->a, h->n_fasta, h->n0, dist, h->min_sites);
    PairStage stage(walk, filter, lamb, beta, precision);
    DeviceBuffer d_state, d_tree;
    if (walk.any()) {
        // the day numbers on the device first: they order the samples of the state
        if ((rc = stage.set_days(days))) return rc;
        if ((rc = d_state.alloc(tracs_anc_state_bytes(n), "state")) || (rc = tracs_anc_init(d_state.ptr, n, stage.days(), nullptr))) return rc;
        if ((rc = walk.begin(true, stage.dense_tc()))) return rc;
        PairColumns c;
        for (Panel pn; walk.more();) {
            if ((rc = walk.next(pn)) || (rc = stage.extract(pn, c))) return rc;
            if (!c.total) continue;
            // a source is chosen by d, filtered d and E(K) ascending, P(direct) descending; -K drops pairs with E(K) above it or NaN
            uint64_t taken = 0;
            if ((rc = tracs_anc_update_coo(d_state.ptr, n, c.total, c.rows, c.cols, weight_column(c, weight), weight == 2 ? 2 : weight == 3 ? 1 : 0,
                                           e_max >= 0.0 ? c.e : nullptr, e_max, c.d, c.nn, c.filt, c.p, c.e, &taken, nullptr))) return rc;
            eligible += taken;
        }
        clock.mark("dense panels + transcluster + ancestor updates");
        size_t nl = 0;
        if ((rc = d_tree.alloc(n * 12, "tree"))) return rc;
        unsigned *t = d_tree.as<unsigned>();
        if ((rc = tracs_anc_emit(d_state.ptr, n, &nl, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, t, t + n, t + 2 * n, nullptr))) return rc;
        TRACS_HIP_CHECK(hipMemcpy(tree.data(), t, n * 12, hipMemcpyDeviceToHost));
        stage.release();
        if (nl && (rc = write_emitted_rows(nl, [&](unsigned *r, unsigned *cc, unsigned *d, unsigned *nn, unsigned *f, double *p, double *e) {
                       return tracs_anc_emit(d_state.ptr, n, &nl, r, cc, d, nn, f, p, e, nullptr, nullptr, nullptr, nullptr); }, writer, days, filter))) return rc;
        clock.mark("ancestor rows: emit, device -> host, format, write");
    }
    rc = writer.close();
    if (rows_written) *rows_written = writer.written();
    if (n_eligible) *n_eligible = eligible;
    if (g_sigint) return interrupted();
    if (rc == TRACS_OK && tree_path) {
        // one line per sample, in order, from parent / root / generation
        std::FILE *fh = std::fopen(tree_path, "ab");
        if (!fh) { set_error(std::string("tracs_distance_ancestors: cannot open ") + tree_path); return TRACS_E_OPEN; }
        for (size_t s = 0; s < n; s++) {
            const uint32_t pa = tree[s], ro = tree[n + s];
            const bool link = pa != 0xFFFFFFFFu && pa < n;
            std::fprintf(fh, "%s,%s,%s,%s,%s,%u,%s\n", h->name_ptr[s], meta_dates[s] ? meta_dates[s] : "", link ? h->name_ptr[pa] : "",
                         link && meta_dates[pa] ? meta_dates[pa] : "", h->name_ptr[ro < n ? ro : s], (unsigned)tree[2 * n + s], ref);
        }
        if (std::fclose(fh) != 0) { set_error(std::string("tracs_distance_ancestors: write failed: ") + tree_path); return TRACS_E_OPEN; }
    }
    return rc;
}

// `tracs distance --tree nj` for one alignment (include/tracs_hip.h: tracs_distance_tree_run).  tree_run is the
// route: the request checked, the main tree, at most one of the two stages below, the files, the counters.
namespace {

struct TreeEdges {
    std::vector<uint32_t> parent, child;
    std::vector<double> length;
    size_t nj = 0, ne = 0;
};

// One tree: the panel walk without a threshold and without the pair rule (every pair has a distance), each dense panel loaded into the
// neighbour-joining state (about n^2 x 8 bytes; the first tree of a call allocates both), the joins on the device, the lengths on the host.
// a == NULL: the zero matrix (a replicate that drew no differing column); acc: NULL (the main tree: stages marked), or the replicates' sums
// kind: the request's -- bit 0 the distance, TRACS_TREE_BIONJ the method, whose state (about 2 n^2 x 8 bytes) and join loop then run
int tree_of_alignment(tracs_alignment *a, const char *const *names, int kind, PanelWalk &walk, DeviceBuffer &d_state, StageClock &clock, double *acc, TreeEdges &t)
{
    int rc;
    const size_t n = walk.n;
    const bool bionj = (kind & TRACS_TREE_BIONJ) != 0;
    std::vector<uint32_t> ja, jb;
    std::vector<double> jd, jra, jrb;
    uint32_t last_ids[3] = {0, n > 1 ? 1u : 0xFFFFFFFFu, 0xFFFFFFFFu};      // (n < 2: no pair exists, nothing runs on the device)
    double last_d[3] = {0.0, 0.0, 0.0};
    t.nj = t.ne = 0;
    if (walk.any()) {
        if (!d_state.ptr && (rc = d_state.alloc(bionj ? tracs_bionj_state_bytes(n) : tracs_nj_state_bytes(n), "state"))) return rc;
        void *const state = d_state.ptr;
        if ((rc = tracs_nj_init(state, n, nullptr))) return rc;
        if (a) {
            walk.a = a;
            walk.at = 0;
            if (!walk.height && (rc = walk.begin(false, false))) return rc;
            for (Panel pn; walk.more();) {
                if ((rc = walk.next(pn)) || (rc = tracs_nj_load_panel(state, n, pn.bd, pn.bn, n, pn.r0, pn.r1, kind & 1, nullptr))) return rc;
            }
        }
        if (acc) lap(clock, acc[0]); else clock.mark("dense panels + matrix load");
        if ((rc = bionj ? tracs_bionj_run(state, n, nullptr) : tracs_nj_run(state, n, nullptr))) return rc;
        TRACS_HIP_CHECK(hipDeviceSynchronize());
        if (g_sigint) return interrupted();
        if (acc) lap(clock, acc[1]); else clock.mark(bionj ? "join loop (bionj)" : "join loop");
        ja.resize(n); jb.resize(n); jd.resize(n); jra.resize(n); jrb.resize(n);
        uint32_t zero[2];
        rc = tracs_nj_emit(state, n, &t.nj, ja.data(), jb.data(), jd.data(), jra.data(), jrb.data(), last_ids, last_d, zero, nullptr);
        if (rc == TRACS_E_ARG && zero[0] < n && zero[1] < n)
            set_error(std::string("samples '") + names[zero[0]] + "' and '" + names[zero[1]] + "' have no site at which both are "
                      "known: no per-site distance (--max-sample-n-share leaves out samples that are mostly N)");
        if (rc) return rc;
    }
    t.parent.resize(2 * n + 1); t.child.resize(2 * n + 1); t.length.resize(2 * n + 1);
    return tracs_nj_edges(n, ja.data(), jb.data(), jd.data(), jra.data(), jrb.data(), last_ids, last_d, t.parent.data(), t.child.data(),
                          t.length.data(), &t.ne);
}

// what a stage learns about the main tree's edges.  Bootstrap: the replicates with the edge's split; transfer: the sums of the transfer
// distances, the lighter sides.  Changes: the Fitch tables; filter: the changes by edge and their verdicts, the edges' kept changes.
struct TreeLabels {
    std::vector<uint32_t> support, light, kept;
    std::vector<uint64_t> sum_phi;
    tracs::FitchTables ft;
    DeviceBuffer d_edge_off, d_edge_site, d_dropped, d_filt;
    tracs::FitchFilter ff = {nullptr, nullptr, nullptr};
    uint64_t kept_sum = 0, edges_dropped = 0;
};

// The replicates (include/tracs_hip.h): the differing columns selected once, then per replicate the draws, the gather into a handle of
// its own, the main tree's walk / load / joins / lengths on the same walk and state, the splits compared and, with r.transfer, its
// program run against the main tree's membership matrix.  One state, one walk, one replicate alive at a time.
int tree_bootstrap_stage(tracs_distance *h, const tracs_tree_request &r, const TreeEdges &t, PanelWalk &walk, DeviceBuffer &d_state, StageClock &clock, TreeLabels &s)
{
    tracs_alignment *a = h->a;
    const size_t n = a->n, L = a->L;
    const char *const *names = h->name_ptr.data();
    const bool transfer = r.transfer != 0;
    int rc;
    s.support.assign(t.ne, 0xFFFFFFFFu);
    s.sum_phi.assign(t.ne, 0); s.light.assign(t.ne, 0);
    if (n < 4) return TRACS_OK;                                            // (no internal edge, nothing to label)
    TreeEdges rep_t;
    std::vector<uint32_t> program(transfer ? 2 * n - 3 : 0);
    DeviceBuffer d_transfer;
    for (size_t e = 0; e < t.ne; e++) if (t.child[e] >= n) s.support[e] = 0;
    if (transfer) {
        if ((rc = d_transfer.alloc(tracs_transfer_state_bytes(n), "transfer")) ||
            (rc = tracs_transfer_init(d_transfer.ptr, n, t.parent.data(), t.child.data(), t.ne, nullptr))) return rc;
        clock.mark("transfer: membership matrix");
    }
    std::vector<uint64_t> differs((L + 63) / 64 + 1, 0);
    size_t V = 0;
    AlignmentOwner var;
    DeviceBuffer d_bits, d_woff, d_w;
    if (L && (rc = site_census(a, nullptr, differs.data(), &V, nullptr))) return rc;
    if (V) {
        tracs_alignment *sel = nullptr;
        if ((rc = select_sites(a, differs.data(), L, UINT32_MAX, &sel, nullptr, nullptr, nullptr, false))) return rc;
        var.reset(sel);
        std::vector<unsigned> bits, woff;
        bootstrap_column_words(differs.data(), L, bits, woff);
        if ((rc = d_bits.upload(bits.data(), bits.size() * 4, "bits")) || (rc = d_woff.upload(woff.data(), woff.size() * 4, "woff")) || (rc = d_w.alloc(V * 4, "w"))) return rc;
    }
    clock.mark("bootstrap: census + differing columns");
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                         // weights + scan + gather; the three stages of a tree (+ support);
                                                                            // transfer: the program on the host, the kernel
    for (uint32_t b = 0; b < r.replicates; b++) {
        if (g_sigint) return interrupted();
        AlignmentOwner rep;
        if (V) {
            tracs_alignment *ra = nullptr;
            if ((rc = bootstrap_weights_launch(L, r.seed, b, d_bits.as<unsigned>(), d_woff.as<unsigned>(), d_w.as<uint32_t>(), V, nullptr)) ||
                (rc = gather_sites(var.get(), d_w.as<uint32_t>(), &ra, nullptr, nullptr, true))) return rc;
            rep.reset(ra);
        }
        lap(clock, acc[0]);
        if ((rc = tree_of_alignment(rep.get(), names, r.kind, walk, d_state, clock, acc + 1, rep_t))) return rc;
        if ((rc = tracs_tree_support(n, t.parent.data(), t.child.data(), t.ne, rep_t.parent.data(), rep_t.child.data(), rep_t.ne, s.support.data()))) return rc;
        if (r.replicate_trees_path && (rc = tracs_tree_write(names, n, rep_t.parent.data(), rep_t.child.data(), rep_t.length.data(), rep_t.ne,
                                                             r.replicate_trees_path, r.ref, nullptr))) return rc;
        lap(clock, acc[3]);
        if (transfer) {
            size_t depth = 0;
            if ((rc = tracs_tree_transfer_program(n, rep_t.parent.data(), rep_t.child.data(), rep_t.ne, program.data(), &depth))) return rc;
            lap(clock, acc[4]);
            if ((rc = transfer_add_program(d_transfer.ptr, n, program.data(), depth, nullptr, nullptr))) return rc;
            lap(clock, acc[5]);
        }
    }
    if (transfer && (rc = tracs_transfer_emit(d_transfer.ptr, n, s.sum_phi.data(), s.light.data()))) return rc;
    if (clock.on) {
        std::fprintf(stderr, "[stage] bootstrap: %u replicates over %zu differing columns\n", (unsigned)r.replicates, V);
        std::fprintf(stderr, "[stage] replicates: weights + scan + gather %.4f s\n", acc[0]);
        std::fprintf(stderr, "[stage] replicates: dense panels + matrix load %.4f s\n", acc[1]);
        std::fprintf(stderr, "[stage] replicates: join loop%s %.4f s\n", (r.kind & TRACS_TREE_BIONJ) ? " (bionj)" : "", acc[2]);
        std::fprintf(stderr, "[stage] replicates: emit, lengths, support %.4f s\n", acc[3]);
        if (transfer)
            std::fprintf(stderr, "[stage] replicates: transfer distances %.4f s (program %.4f s, kernel %.4f s)\n", acc[4] + acc[5], acc[4], acc[5]);
    }
    return TRACS_OK;
}

// The Fitch count pass on the main tree (include/tracs_hip.h); a total above r.max_entries is refused here, before any file is touched.
// r.filter: the changes regrouped by edge and the recombination filter's window test on every edge's list.
int tree_changes_stage(tracs_distance *h, const tracs_tree_request &r, const TreeEdges &t, StageClock &clock, TreeLabels &c)
{
    const size_t n = h->a->n;
    int rc;
    clock.memory("before the Fitch passes");                               // (the tree's matrix is gone; under the iteration it, the walk's
                                                                           // panels and the clone stay until the loop ends)
    if (n && (rc = tracs::fitch_tables(h->a, t.parent.data(), t.child.data(), t.ne, c.ft))) return rc;
    clock.mark("tree changes: count pass, offsets");
    if (g_sigint) return interrupted();
    if ((r.changes_path || r.filter) && c.ft.total > r.max_entries) {      // (the edge lists and their verdicts hold one entry per change)
        set_error("the tree has " + std::to_string(c.ft.total) + " changes in all, more than --max-entries " + std::to_string(r.max_entries) +
                  "; nothing was written");
        return TRACS_E_ARG;
    }
    c.kept.assign(std::max<size_t>(t.ne, 1), 0);
    if (r.filter && n && t.ne) {
        const size_t total = (size_t)c.ft.total;
        if ((rc = c.d_edge_off.alloc((t.ne + 1) * 8, "edge_off")) || (rc = c.d_edge_site.alloc(std::max<size_t>(total, 1) * 4, "edge_site")) ||
            (rc = c.d_dropped.alloc(std::max<size_t>(total, 1), "dropped")) || (rc = c.d_filt.alloc(t.ne * 4, "filt"))) return rc;
        if ((rc = tracs_fitch_edge_sites(h->a, t.parent.data(), t.child.data(), t.ne, c.ft.d_edge.get(), c.d_edge_off.as<int64_t>(),
                                         c.d_edge_site.as<uint32_t>(), total, nullptr))) return rc;
        clock.mark("tree filter: the changes by edge");
        if ((rc = tracs_filter_recomb_lists(h->a, c.d_edge_off.as<int64_t>(), c.d_edge_site.as<uint32_t>(), t.ne, total, c.d_filt.as<uint32_t>(),
                                            c.d_dropped.as<uint8_t>(), nullptr))) return rc;
        TRACS_HIP_CHECK(hipMemcpy(c.kept.data(), c.d_filt.ptr, t.ne * 4, hipMemcpyDeviceToHost));
        clock.mark("tree filter: window test on the edges' lists");
        for (size_t e = 0; e < t.ne; e++) {
            c.kept_sum += c.kept[e];
            c.edges_dropped += c.kept[e] < c.ft.edge_changes[e];
        }
        c.ff = {c.d_edge_off.as<long long>(), c.d_edge_site.as<unsigned>(), c.d_dropped.as<uint8_t>()};
        if (g_sigint) return interrupted();
    }
    c.ft.edge_changes.resize(std::max<size_t>(t.ne, 1), 0);
    return TRACS_OK;
}

// One tree's row of the iterations file (include/tracs_hip.h: tracs_distance_tree_iterate)
struct TreeIterRow {
    uint64_t changes, kept, edges_dropped, masked;
    bool has_masked;
    int64_t shared;                                                        // -1: NA
    int32_t same_as;                                                       // -1: NA
};

// the non-trivial splits of `t` that `other` has (tracs_tree_support's comparison); n < 4: there is none
int tree_shared_splits(size_t n, const TreeEdges &t, const TreeEdges &other, size_t &shared)
{
    shared = 0;
    if (n < 4) return TRACS_OK;
    std::vector<uint32_t> count(t.ne, 0);
    const int rc = tracs_tree_support(n, t.parent.data(), t.child.data(), t.ne, other.parent.data(), other.child.data(), other.ne, count.data());
    for (size_t e = 0; e < t.ne; e++) if (t.child[e] >= n) shared += count[e];
    return rc;
}

// The branch filter iterated into the topology (include/tracs_hip.h: tracs_distance_tree_iterate).  t comes in as T_0 and
// goes out as the final tree, ch as its labels: the changes stage runs on every T_k with the handle's own alignment, its verdicts mask
// one clone (restored from the handle's planes between iterations), and the clone goes through the main tree's walk, state and joins as
// a bootstrap replicate does.  Earlier trees stay on the host for the split comparison.
int tree_iterate_stage(tracs_distance *h, const tracs_tree_request &r, const tracs_tree_iterate &it, PanelWalk &walk, DeviceBuffer &d_state,
                       StageClock &clock, TreeEdges &t, std::unique_ptr<TreeLabels> &ch, std::vector<TreeIterRow> &rows,
                       tracs_tree_iterate_result &ires)
{
    const size_t n = h->a->n;
    const char *const *names = h->name_ptr.data();
    const bool has_planes = tracs_alignment_bytes(h->a) != 0;
    std::vector<TreeEdges> seen;
    AlignmentOwner clone;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};                                  // the two stages of a tree; clone / restore; the mask
    uint32_t k = 0;
    bool stop = false;
    int32_t same = -1;
    int64_t shared_prev = -1;
    int rc;
    ires = tracs_tree_iterate_result();
    ires.same_as = -1;
    for (;;) {
        ch.reset(new TreeLabels());
        if ((rc = tree_changes_stage(h, r, t, clock, *ch))) return rc;
        TreeIterRow row = {ch->ft.total, ch->kept_sum, ch->edges_dropped, 0, false, shared_prev, -1};
        if (stop) {
            row.same_as = same;
            rows.push_back(row);
            break;
        }
        // M_{k + 1}: the handle's planes, then the verdicts of T_k
        uint64_t cells = 0, work = 0;
        if (has_planes) {
            if (!clone) {
                tracs_alignment *c = nullptr;
                if ((rc = tracs_alignment_clone(h->a, &c, nullptr))) return rc;
                clone.reset(c);
            } else if ((rc = copy_planes("tracs_distance_tree_iterate", clone.get(), h->a, nullptr))) return rc;
            lap(clock, acc[2]);
            if (ch->d_dropped.ptr && ch->ft.total &&
                (rc = mask_subtrees(clone.get(), t.parent.data(), t.child.data(), t.ne, ch->d_edge_off.as<int64_t>(), ch->d_edge_site.as<uint32_t>(),
                                    ch->d_dropped.as<uint8_t>(), (size_t)ch->ft.total, &cells, &work, nullptr))) return rc;
            lap(clock, acc[3]);
        }
        row.masked = cells; row.has_masked = true;
        rows.push_back(row);
        ires.masked_cells_last = cells;
        ires.mask_work_max = std::max<uint64_t>(ires.mask_work_max, work);
        ch.reset();                                                        // (the Fitch tables and lists of T_k go before the next matrix)
        seen.emplace_back(std::move(t));
        t = TreeEdges();
        k++;
        if (g_sigint) return interrupted();
        // T_k = NJ(M_k)
        if ((rc = tree_of_alignment(has_planes ? clone.get() : h->a, names, r.kind, walk, d_state, clock, acc, t))) {
            if (rc == TRACS_E_ARG) set_error("iteration " + std::to_string(k) + " of --tree-iterate: " + std::string(tracs_last_error()));
            return rc;
        }
        same = -1;
        size_t shared = 0;
        for (size_t j = 0; j < seen.size(); j++) {                         // (the smallest j with T_k's splits; then T_{k-1} alone)
            if (same >= 0 && j + 1 < seen.size()) continue;
            if ((rc = tree_shared_splits(n, t, seen[j], shared))) return rc;
            if (same < 0 && (n < 4 || shared == n - 3)) same = (int32_t)j;
        }
        shared_prev = (int64_t)shared;                                     // (the last comparison is the one with T_{k-1})
        stop = same >= 0 || k >= it.max_iterations;
    }
    ires.iterations = k;
    ires.same_as = same;
    if (clock.on) {
        std::fprintf(stderr, "[stage] iterations: %u trees after the first, %s\n", (unsigned)k,
                     same < 0 ? "stopped at the limit" : same + 1 == (int32_t)k ? "converged" : "a cycle");
        std::fprintf(stderr, "[stage] iterations: clone / restore %.4f s\n", acc[2]);
        std::fprintf(stderr, "[stage] iterations: mask %.4f s (largest W %llu)\n", acc[3], (unsigned long long)ires.mask_work_max);
        std::fprintf(stderr, "[stage] iterations: dense panels + matrix load %.4f s\n", acc[0]);
        std::fprintf(stderr, "[stage] iterations: join loop%s %.4f s\n", (r.kind & TRACS_TREE_BIONJ) ? " (bionj)" : "", acc[1]);
    }
    return TRACS_OK;
}

int tree_run(const std::string &who, tracs_distance *h, const tracs_tree_request &r, tracs_tree_result &res,
             const tracs_tree_iterate *it = nullptr, tracs_tree_iterate_result *ires = nullptr)
{
    // (a) the request
    res = tracs_tree_result();
    tracs_tree_iterate_result ires_none;
    tracs_tree_iterate_result &ir = ires ? *ires : ires_none;
    ir = tracs_tree_iterate_result();
    ir.same_as = -1;
    const bool boot = r.replicates || r.transfer || r.replicate_trees_path, changes = r.changes || r.filter;
    if (!h || !h->a || !r.path || !r.ref) { set_error(who + ": NULL argument"); return TRACS_E_ARG; }
    if (boot && changes) {
        set_error(who + ": the changes on the tree and bootstrap replicates cannot be combined yet (the tree is reproducible bit for bit: "
                        "run once with each and join the two --tree-edges files on parent and child)");
        return TRACS_E_ARG;
    }
    if (it && (!r.filter || boot)) { set_error(who + ": the iteration needs the branch filter (filter != 0) and takes no replicates"); return TRACS_E_ARG; }
    if (it && (it->max_iterations < 1 || it->max_iterations > 100)) { set_error(who + ": max_iterations must be in [1, 100]"); return TRACS_E_ARG; }
    if (boot && (r.kind & ~TRACS_TREE_BIONJ) != 0) { set_error(who + ": bootstrap replicates take the SNP distance (kind 0) only"); return TRACS_E_ARG; }
    if (r.kind < 0 || r.kind > (1 | TRACS_TREE_BIONJ)) { set_error(who + ": kind must be 0 (snp) or 1 (per-site)"); return TRACS_E_ARG; }
    if (boot && r.replicates < 1) { set_error(who + ": at least one replicate"); return TRACS_E_ARG; }
    if (h->n_fasta != 1) { set_error(who + ": a tree joins the samples of one alignment"); return TRACS_E_ARG; }
    SigintScope sigint;
    const size_t n = h->a->n;
    const char *const *names = h->name_ptr.data();
    // (the BIONJ state has the same limit)
    if (n && !tracs_nj_state_bytes(n)) { set_error(who + ": too many samples for one distance matrix"); return TRACS_E_ARG; }
    if (boot && h->a->L >= 0xFFFFFFFFull) { set_error(who + ": too many columns"); return TRACS_E_ARG; }
    StageClock clock;
    int rc;
    // (b) the main tree
    TreeEdges t;
    PanelWalk walk(h->a, 1, n, 2147483647, 0);
    DeviceBuffer d_state;
    if ((rc = tree_of_alignment(h->a, names, r.kind, walk, d_state, clock, nullptr, t))) return rc;
    // (c) at most one stage.  The replicates are joined on the main tree's walk and state, which stay until the call returns; the Fitch
    // passes need neither, so both go first: at n = 10000 the state alone is 0.8 GB that must not sit under them.
    std::unique_ptr<TreeLabels> labels(new TreeLabels());
    std::vector<TreeIterRow> iter_rows;
    if (boot && (rc = tree_bootstrap_stage(h, r, t, walk, d_state, clock, *labels))) return rc;
    if (it) {                                                              // (the walk and the state stay: every iteration joins on them)
        if ((rc = tree_iterate_stage(h, r, *it, walk, d_state, clock, t, labels, iter_rows, ir))) {
            ir = tracs_tree_iterate_result();                              // (a run that failed reports nothing of its iterations)
            ir.same_as = -1;
            return rc;
        }
        walk.d_dist.release(); walk.d_nn.release(); d_state.release();
    } else if (changes) {
        walk.d_dist.release(); walk.d_nn.release(); d_state.release();
        if ((rc = tree_changes_stage(h, r, t, clock, *labels))) return rc;
    }
    TreeLabels &ch = *labels;
    // (d) the files
    const uint32_t *edge_changes = changes ? ch.ft.edge_changes.data() : nullptr, *kept = r.filter ? ch.kept.data() : nullptr;
    const uint32_t *const parent = t.parent.data(), *const child = t.child.data();
    if (changes && r.create) {                                             // (tracs/distance.py leaves the run's files to the library then)
        const std::pair<const char *, std::string> made[6] = {{r.path, ""}, {r.edges_path, tree_edges_header({nullptr, nullptr, edge_changes, kept})},
            {it ? it->iterations_path : nullptr, "iteration,changes,kept,dropped,branches with a drop,masked cells,shared splits,same as,MSA file\n"},
            {r.changes_path, std::string("parent,child,contig,position,alleleParent,alleleChild,") + (r.filter ? "dropped," : "") + "MSA file\n"},
            {r.sites_path, "contig,position,changes,minimum,MSA file\n"}, {r.filtered_path, ""}};
        for (const auto &f : made) {
            if (!f.first) continue;
            std::FILE *fh = std::fopen(f.first, "wb");
            if (!fh || std::fputs(f.second.c_str(), fh) < 0 || std::fclose(fh) != 0) { set_error(std::string("cannot write ") + f.first); return TRACS_E_OPEN; }
        }
    }
    if (r.filter) rc = tracs_tree_write_filtered(names, n, parent, child, t.length.data(), t.ne, edge_changes, kept, r.path, r.ref, r.edges_path);
    else if (changes) rc = tracs_tree_write_changes(names, n, parent, child, t.length.data(), t.ne, edge_changes, r.path, r.ref, r.edges_path);
    else if (r.transfer) rc = tracs_tree_write_transfer(names, n, parent, child, t.length.data(), t.ne, ch.support.data(), ch.sum_phi.data(),
                                                        ch.light.data(), r.replicates, r.path, r.ref, r.edges_path);
    else if (boot) rc = tracs_tree_write_support(names, n, parent, child, t.length.data(), t.ne, ch.support.data(), r.replicates, r.path, r.ref, r.edges_path);
    else rc = tracs_tree_write(names, n, parent, child, t.length.data(), t.ne, r.path, r.ref, r.edges_path);
    if (!rc && r.filter && r.filtered_path) {
        const std::vector<double> kept_length(ch.kept.begin(), ch.kept.end());
        rc = tracs_tree_write(names, n, parent, child, kept_length.data(), t.ne, r.filtered_path, r.ref, nullptr);
    }
    if (rc) return rc;
    if (it && it->iterations_path) {
        std::FILE *fh = std::fopen(it->iterations_path, "ab");
        if (!fh) { set_error(std::string("cannot open ") + it->iterations_path + " for appending"); return TRACS_E_OPEN; }
        const auto na = [](bool have, long long v) { return have ? std::to_string(v) : std::string("NA"); };
        for (size_t k = 0; k < iter_rows.size(); k++) {
            const TreeIterRow &w = iter_rows[k];
            std::fprintf(fh, "%zu,%llu,%llu,%llu,%llu,%s,%s,%s,%s\n", k, (unsigned long long)w.changes, (unsigned long long)w.kept,
                         (unsigned long long)(w.changes - w.kept), (unsigned long long)w.edges_dropped, na(w.has_masked, (long long)w.masked).c_str(),
                         na(w.shared >= 0, w.shared).c_str(), na(w.same_as >= 0, w.same_as).c_str(), r.ref);
        }
        if (std::fclose(fh) != 0) { set_error(std::string("write failed: ") + it->iterations_path); return TRACS_E_OPEN; }
    }
    clock.mark("tree: emit, lengths, format, write");
    if (changes) {
        if (n && (rc = tracs::fitch_write(h->a, names, h->kept.empty() ? nullptr : h->kept.data(), h->source_len, parent, child, t.ne, ch.ft,
                                          r.changes_path, r.sites_path, r.ref, r.contig_names, r.contig_lengths, r.n_contigs, r.n_threads,
                                          ch.ff.d_dropped ? &ch.ff : nullptr)))
            return rc;
        clock.mark("tree changes: fill, device -> host, format, write");
        clock.memory("after the Fitch passes");
    }
    // (e) the counters
    res = {t.nj, r.edges_path ? t.ne : 0, ch.ft.total, ch.ft.sum_minimum, ch.kept_sum, ch.edges_dropped};
    if (g_sigint) return interrupted();
    return TRACS_OK;
}

// the five older entry points: their arguments as a request (its first fields in order, the others 0), the result into their out-parameters
int tree_run_out(const char *who, tracs_distance *h, const tracs_tree_request &r, std::initializer_list<uint64_t *> out)
{
    tracs_tree_result res;
    const int rc = tree_run(who, h, r, res);
    const uint64_t field[6] = {res.n_joins, res.rows_written, res.n_changes, res.sum_minimum, res.n_kept, res.n_edges_dropped};
    size_t k = 0;
    for (uint64_t *p : out) { if (p) *p = field[k]; k++; }
    return rc;
}

}  // namespace

int tracs_distance_tree_run(tracs_distance *h, const tracs_tree_request *req, tracs_tree_result *res)
{
    tracs_tree_result none = {};
    if (res) *res = none;
    if (!req) { set_error("tracs_distance_tree_run: NULL argument"); return TRACS_E_ARG; }
    return tree_run("tracs_distance_tree_run", h, *req, res ? *res : none);
}

int tracs_distance_tree_iterate(tracs_distance *h, const tracs_tree_request *req, const tracs_tree_iterate *it, tracs_tree_result *res,
                                tracs_tree_iterate_result *ires)
{
    tracs_tree_result none = {};
    if (res) *res = none;
    if (ires) { *ires = tracs_tree_iterate_result(); ires->same_as = -1; }
    if (!req) { set_error("tracs_distance_tree_iterate: NULL argument"); return TRACS_E_ARG; }
    return tree_run(it ? "tracs_distance_tree_iterate" : "tracs_distance_tree_run", h, *req, res ? *res : none, it, ires);
}

int tracs_distance_tree(tracs_distance *h, int kind, const char *path, const char *ref, const char *edges_path, uint64_t *n_joins,
                        uint64_t *rows_written)
{
    return tree_run_out("tracs_distance_tree", h, {kind, path, ref, edges_path}, {n_joins, rows_written});
}

int tracs_distance_tree_changes(tracs_distance *h, int kind, const char *path, const char *ref, const char *edges_path, const char *changes_path,
                                const char *sites_path, const char *const *contig_names, const uint64_t *contig_lengths, size_t n_contigs,
                                uint64_t max_entries, int n_threads, int create, uint64_t *n_joins, uint64_t *rows_written, uint64_t *n_changes,
                                uint64_t *sum_minimum)
{
    tracs_tree_request r = {kind, path, ref, edges_path};
    r.changes = 1; r.changes_path = changes_path; r.sites_path = sites_path; r.contig_names = contig_names; r.contig_lengths = contig_lengths;
    r.n_contigs = n_contigs; r.max_entries = max_entries; r.n_threads = n_threads; r.create = create;
    return tree_run_out("tracs_distance_tree_changes", h, r, {n_joins, rows_written, n_changes, sum_minimum});
}

int tracs_distance_tree_filter(tracs_distance *h, int kind, const char *path, const char *ref, const char *edges_path, const char *changes_path,
                               const char *sites_path, const char *filtered_path, const char *const *contig_names, const uint64_t *contig_lengths,
                               size_t n_contigs, uint64_t max_entries, int n_threads, int create, uint64_t *n_joins, uint64_t *rows_written,
                               uint64_t *n_changes, uint64_t *sum_minimum, uint64_t *n_kept, uint64_t *n_edges_dropped)
{
    tracs_tree_request r = {kind, path, ref, edges_path};
    r.changes = r.filter = 1; r.changes_path = changes_path; r.sites_path = sites_path; r.filtered_path = filtered_path; r.contig_names = contig_names;
    r.contig_lengths = contig_lengths; r.n_contigs = n_contigs; r.max_entries = max_entries; r.n_threads = n_threads; r.create = create;
    return tree_run_out("tracs_distance_tree_filter", h, r, {n_joins, rows_written, n_changes, sum_minimum, n_kept, n_edges_dropped});
}

int tracs_distance_tree_bootstrap(tracs_distance *h, int kind, const char *path, const char *ref, const char *edges_path, uint32_t replicates,
                                  uint64_t seed, const char *replicate_trees_path, uint64_t *n_joins, uint64_t *rows_written)
{
    // (no replicates: a plain tree to a request, a refusal here -- as transfer support without replicates it stays one)
    return tree_run_out("tracs_distance_tree_bootstrap", h, {kind, path, ref, edges_path, replicates, seed, !replicates, replicate_trees_path},
                        {n_joins, rows_written});
}

int tracs_distance_tree_bootstrap_transfer(tracs_distance *h, int kind, const char *path, const char *ref, const char *edges_path,
                                           uint32_t replicates, uint64_t seed, const char *replicate_trees_path, uint64_t *n_joins,
                                           uint64_t *rows_written)
{
    return tree_run_out("tracs_distance_tree_bootstrap_transfer", h, {kind, path, ref, edges_path, replicates, seed, 1, replicate_trees_path},
                        {n_joins, rows_written});
}

// `tracs distance --histogram` for one alignment (include/tracs_hip.h): the panel walk of tracs_distance_run with
// tracs_hist_update on each dense panel instead of the rows; with --filter the panel's pairs within the threshold are extracted and
// filtered by the same pair stage, and a second state counts their filtered distances.  What crosses to the host is the
// non-empty bins.
int tracs_distance_histogram(tracs_distance *h, int dist, int filter, const int32_t *group, const char *path, const char *ref,
                             uint64_t *n_eligible, uint64_t *rows_written)
{
    if (rows_written) *rows_written = 0;
    if (n_eligible) *n_eligible = 0;
    if (!h || !h->a || !path || !ref) { set_error("tracs_distance_histogram: NULL argument"); return TRACS_E_ARG; }
    if (dist < 0) { set_error("tracs_distance_histogram: dist must not be negative"); return TRACS_E_ARG; }
    SigintScope sigint;
    const size_t n = h->a->n;
    const size_t n_bins = std::min<size_t>(h->a->L, (size_t)dist) + 1;  // d <= L and d <= dist: no eligible value falls outside
    FILE *fp = std::fopen(path, "ab");
    if (!fp) { set_error(std::string("cannot open ") + path + " for appending"); return TRACS_E_OPEN; }
    struct Closer { FILE *&f; ~Closer() { if (f) std::fclose(f); } } closer{fp};
    StageClock clock;
    uint64_t eligible = 0, written = 0;
    PanelWalk walk(h->a, h->n_fasta, h->n0, dist, h->min_sites);
    PairStage stage(walk, filter);                                   // (used only under --filter: five uint32 columns, no dates)
    DeviceBuffer d_state[2], d_group, d_val, d_cnt;
    if (walk.any()) {
        int rc;
        const int n_states = filter ? 2 : 1;
        for (int s = 0; s < n_states; s++)
            if ((rc = d_state[s].alloc(tracs_hist_state_bytes(n_bins), "state")) || (rc = tracs_hist_init(d_state[s].ptr, n_bins, nullptr))) return rc;
        if ((rc = walk.begin(filter != 0, false))) return rc;
        if (group && (rc = d_group.upload(group, n * 4, "group"))) return rc;
        PairColumns c;
        for (Panel pn; walk.more();) {
            if ((rc = walk.next(pn))) return rc;
            if ((rc = tracs_hist_update(pn.bd, n, n, pn.r0, pn.r1, walk.j_start, dist, d_group.as<int>(), d_state[0].ptr, n_bins, nullptr))) return rc;
            if (!filter) continue;
            // the filtered distances of the panel's eligible pairs (src/pairsnp.hpp:405-413), as tracs_distance_run takes them
            if ((rc = stage.extract(pn, c))) return rc;
            if (c.total && (rc = tracs_hist_update_coo(c.rows, c.cols, c.filt, c.total, d_group.as<int>(), d_state[1].ptr, n_bins, nullptr))) return rc;
        }
        clock.mark("dense panels + histogram updates");
        static const char *const column[2] = {"snp", "filter"};
        std::string text;
        for (int s = 0; s < n_states; s++) {
            size_t nr = 0;
            if ((rc = tracs_hist_emit(d_state[s].ptr, n_bins, &nr, nullptr, nullptr, nullptr, nullptr, nullptr))) return rc;
            if (!nr) continue;
            if ((rc = d_val.alloc(nr * 4, "val")) || (rc = d_cnt.alloc(nr * 8 * 3, "cnt"))) return rc;
            uint64_t *cnt = d_cnt.as<uint64_t>();
            if ((rc = tracs_hist_emit(d_state[s].ptr, n_bins, &nr, d_val.as<unsigned>(), cnt, cnt + nr, cnt + 2 * nr, nullptr))) return rc;
            std::vector<uint32_t> hv(nr);
            std::vector<uint64_t> hc(nr * 3);
            TRACS_HIP_CHECK(hipMemcpy(hv.data(), d_val.ptr, nr * 4, hipMemcpyDeviceToHost));
            TRACS_HIP_CHECK(hipMemcpy(hc.data(), cnt, nr * 24, hipMemcpyDeviceToHost));
            char line[160];
            for (size_t t = 0; t < nr; t++) {
                const int k = std::snprintf(line, sizeof line, "%s,%u,%llu,%llu,%llu,", column[s], hv[t], (unsigned long long)hc[t],
                                            (unsigned long long)hc[nr + t], (unsigned long long)hc[2 * nr + t]);
                text.append(line, (size_t)k);
                text.append(ref);
                text.push_back('\n');
                if (s == 0) eligible += hc[t] + hc[nr + t] + hc[2 * nr + t];
            }
            written += nr;
        }
        if (!text.empty() && std::fwrite(text.data(), 1, text.size(), fp) != text.size()) {
            set_error(std::string("write to ") + path + " failed");
            return TRACS_E_OPEN;
        }
        clock.mark("histogram rows: emit, device -> host, format, write");
    }
    const int rc_close = std::fclose(fp);
    fp = nullptr;
    if (rc_close != 0) { set_error(std::string("write to ") + path + " failed"); return TRACS_E_OPEN; }
    if (rows_written) *rows_written = written;
    if (n_eligible) *n_eligible = eligible;
    if (g_sigint) return interrupted();
    return TRACS_OK;
}

size_t tracs_pairsnp_len(const tracs_pairsnp_result *r) { return r ? r->rows.size() : 0; }
size_t tracs_pairsnp_nseq(const tracs_pairsnp_result *r) { return r ? r->nseq : 0; }
size_t tracs_pairsnp_seqlen(const tracs_pairsnp_result *r) { return r ? r->L : 0; }
const uint64_t *tracs_pairsnp_rows(const tracs_pairsnp_result *r) { return r ? r->rows.data() : nullptr; }
const uint64_t *tracs_pairsnp_cols(const tracs_pairsnp_result *r) { return r ? r->cols.data() : nullptr; }
const uint64_t *tracs_pairsnp_distances(const tracs_pairsnp_result *r) { return r ? r->dist.data() : nullptr; }
const uint64_t *tracs_pairsnp_filt_distances(const tracs_pairsnp_result *r) { return r ? r->filt.data() : nullptr; }
const uint64_t *tracs_pairsnp_ncompared(const tracs_pairsnp_result *r) { return r ? r->ncomp.data() : nullptr; }
const char *tracs_pairsnp_name(const tracs_pairsnp_result *r, size_t i) { return (r && i < r->names.size()) ? r->names[i].c_str() : nullptr; }
void tracs_pairsnp_free(tracs_pairsnp_result *r) { delete r; }

}  // extern "C"
