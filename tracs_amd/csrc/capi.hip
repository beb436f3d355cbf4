// capi.hip -- library-wide state (error slot, scratch pool) and the host-level pairsnp entry.
//
// tracs_pairsnp restates the DRIVER part of /root/reference/src/pairsnp.hpp:320-457:
// argument check (:340-343), one- vs two-file pair ranges (:352-360), the output tuple (:451-457).
// The arithmetic is in pairsnp.hip.
#include "common.h"
#include "fasta.h"
#include "rowwriter.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace tracs {

static thread_local std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }

struct Scratch { void *ptr = nullptr; size_t bytes = 0; };
constexpr int kScratchSlots = 96;
static Scratch g_scratch[8][kScratchSlots];
static std::mutex g_scratch_mu;

int workspace_get(int slot, size_t bytes, void **out)
{
    int dev = 0;
    TRACS_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 8 || slot < 0 || slot >= kScratchSlots) { set_error("workspace_get: bad device/slot"); return TRACS_E_ARG; }
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    Scratch &s = g_scratch[dev][slot];
    if (s.bytes < bytes) {
        if (s.ptr) { TRACS_HIP_CHECK(hipDeviceSynchronize()); TRACS_HIP_CHECK(hipFree(s.ptr)); s.ptr = nullptr; s.bytes = 0; }
        const size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&s.ptr, want);
        if (e != hipSuccess) { s.ptr = nullptr; set_error(std::string("hipMalloc(workspace): ") + hipGetErrorString(e)); return TRACS_E_NOMEM; }
        s.bytes = want;
    }
    *out = s.ptr;
    return TRACS_OK;
}

static std::recursive_mutex g_call_mu[8];
static hipStream_t g_last_stream[8];
static bool g_have_stream[8];
static bool g_caller_orders_streams = false;     // tracs_set_stream_policy

DeviceCall::DeviceCall(hipStream_t stream) : dev(0)
{
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 8) dev = 0;
    g_call_mu[dev].lock();
    if (g_have_stream[dev] && g_last_stream[dev] != stream && !g_caller_orders_streams) (void)hipDeviceSynchronize();
    g_last_stream[dev] = stream;
    g_have_stream[dev] = true;
}
DeviceCall::~DeviceCall() { g_call_mu[dev].unlock(); }

void workspace_release_all()
{
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    for (auto &dev : g_scratch)
        for (auto &s : dev)
            if (s.ptr) { (void)hipFree(s.ptr); s.ptr = nullptr; s.bytes = 0; }
}

}  // namespace tracs

using namespace tracs;

// TRACS_STAGE_TRACE=1: wall time of the stages of the host-level entry points on stderr, one "[stage] name seconds" line each
// (scripts/bench_e2e.py collects them into the end-to-end table of DESIGN.md 5)
struct StageClock {
    bool on;
    std::chrono::steady_clock::time_point t;
    StageClock() : on(std::getenv("TRACS_STAGE_TRACE") != nullptr), t(std::chrono::steady_clock::now()) {}
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
};

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
        unsigned *d_counts = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_counts), n * 4);
        if (e != hipSuccess) { (void)hipGetLastError(); set_error(std::string("hipMalloc(sample counts): ") + hipGetErrorString(e)); return TRACS_E_NOMEM; }
        int rc = sample_n_counts(a, rule->keep, rule->keep_len, d_counts, nullptr);
        if (!rc && (e = hipMemcpy(src.n_count.data(), d_counts, n * 4, hipMemcpyDeviceToHost)) != hipSuccess) {
            set_error(std::string("hipMemcpy(sample counts): ") + hipGetErrorString(e));
            rc = TRACS_E_HIP;
        }
        (void)hipFree(d_counts);
        if (rc) return rc;
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

static int pairsnp_run(const char *const *fasta, int n_fasta, int dist, int filter, SiteRule *rule, tracs_pairsnp_result **out)
{
    if (!out) { set_error("tracs_pairsnp: out is NULL"); return TRACS_E_ARG; }
    *out = nullptr;
    if (n_fasta < 1 || n_fasta > 2 || !fasta) { set_error("Invalid number of fasta files!"); return TRACS_E_ARG; }   // :340-343
    SigintScope sigint;
    tracs_alignment *a = nullptr;
    char *names = nullptr;
    size_t names_bytes = 0, n0 = 0;
    int rc = alignment_from_fasta_sites(fasta, n_fasta, &a, &names, &names_bytes, &n0, rule);
    if (rc) return rc;
    auto *res = new tracs_pairsnp_result();
    res->nseq = a->n; res->L = a->L;
    if (rule) res->source = std::move(rule->source);
    else res->source.rule_sites = a->L;
    const uint32_t min_sites = rule ? rule->min_sites : 0;
    { size_t o = 0; for (size_t i = 0; i < a->n; i++) { res->names.emplace_back(names + o); o += res->names.back().size() + 1; } }
    tracs_free(names);
    // pair ranges (:348-360)
    const size_t n = a->n;
    const size_t i_end = n_fasta == 1 ? n : n0;
    const size_t j_start = n_fasta == 1 ? 0 : n0;

    unsigned *d_dist = nullptr, *d_nn = nullptr, *d_rows = nullptr, *d_cols = nullptr, *d_d = nullptr, *d_n = nullptr;
    unsigned *d_filt = nullptr;
    long long *d_off = nullptr;
    size_t pair_cap = 0;
    auto cleanup = [&]() {
        void *p[] = {d_dist, d_nn, d_rows, d_cols, d_d, d_n, d_off, d_filt};
        for (void *q : p) if (q) (void)hipFree(q);
        tracs_alignment_free(a);
    };
#define PS_CHECK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { cleanup(); delete res; set_error(std::string(#x ": ") + hipGetErrorString(e__)); return TRACS_E_HIP; } } while (0)
#define PS_RC(x) do { int r__ = (x); if (r__) { cleanup(); delete res; return r__; } } while (0)
    StageClock clock;
    double t_dense = 0.0, t_coo = 0.0, t_pull = 0.0, t_filter = 0.0;
    auto lap = [&](double &acc) {
        if (!clock.on) return;
        (void)hipDeviceSynchronize();
        const auto now = std::chrono::steady_clock::now();
        acc += std::chrono::duration<double>(now - clock.t).count();
        clock.t = now;
    };
    if (n >= 2 && i_end > 0) {
        // row panels bounded to ~1 GiB per dense matrix
        const size_t panel = std::max<size_t>(64, std::min<size_t>(i_end, (1ull << 28) / std::max<size_t>(n, 1)));
        PS_CHECK(hipMalloc(reinterpret_cast<void **>(&d_dist), panel * n * 4));
        PS_CHECK(hipMalloc(reinterpret_cast<void **>(&d_nn), panel * n * 4));
        PS_CHECK(hipMalloc(reinterpret_cast<void **>(&d_off), (panel + 1) * 8));
        size_t cap = 0;
        std::vector<unsigned> h32;
        for (size_t r0 = 0; r0 < i_end; r0 += panel) {
            if (g_sigint) { cleanup(); delete res; set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }
            const size_t r1 = std::min(i_end, r0 + panel);
            // the dense block is addressed as base[(i) * ld + j] with i absolute: shift the base
            unsigned *bd = d_dist - r0 * n, *bn = d_nn - r0 * n;
            lap(t_pull);
            PS_RC(tracs_pairsnp_dense_thr(a, r0, r1, j_start, bd, bn, n, dist, nullptr));   // early out beyond `dist`
            if (min_sites) PS_RC(pairs_min_sites(bd, bn, n, n, r0, r1, j_start, dist, min_sites, nullptr));
            lap(t_dense);
            PS_RC(tracs_coo_count(bd, n, n, r0, r1, j_start, dist, reinterpret_cast<int64_t *>(d_off), nullptr));
            long long total = 0;
            PS_CHECK(hipMemcpy(&total, d_off + (r1 - r0), 8, hipMemcpyDeviceToHost));
            if (total <= 0) continue;
            if ((size_t)total > cap) {
                void *p[] = {d_rows, d_cols, d_d, d_n};
                for (void *q : p) if (q) PS_CHECK(hipFree(q));
                d_rows = d_cols = d_d = d_n = nullptr;
                cap = (size_t)total;
                PS_CHECK(hipMalloc(reinterpret_cast<void **>(&d_rows), cap * 4));
                PS_CHECK(hipMalloc(reinterpret_cast<void **>(&d_cols), cap * 4));
                PS_CHECK(hipMalloc(reinterpret_cast<void **>(&d_d), cap * 4));
                PS_CHECK(hipMalloc(reinterpret_cast<void **>(&d_n), cap * 4));
            }
            PS_RC(tracs_coo_fill(bd, bn, n, n, r0, r1, j_start, dist, reinterpret_cast<int64_t *>(d_off), d_rows, d_cols, d_d, d_n, nullptr));
            lap(t_coo);
            h32.resize((size_t)total);
            auto pull = [&](unsigned *src, std::vector<uint64_t> &dst) -> hipError_t {
                hipError_t e = hipMemcpy(h32.data(), src, (size_t)total * 4, hipMemcpyDeviceToHost);
                if (e != hipSuccess) return e;
                widen_append(dst, h32.data(), (size_t)total);
                return hipSuccess;
            };
            PS_CHECK(pull(d_rows, res->rows));
            PS_CHECK(pull(d_cols, res->cols));
            PS_CHECK(pull(d_d, res->dist));
            PS_CHECK(pull(d_n, res->ncomp));
            lap(t_pull);
            if (filter) {
                // recombination filter on the pairs just emitted (:405-413): SNP sites from the samples' departure lists
                if (g_sigint) { cleanup(); delete res; set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }
                if ((size_t)total > pair_cap) {
                    if (d_filt) PS_CHECK(hipFree(d_filt));
                    d_filt = nullptr;
                    pair_cap = (size_t)total + (size_t)total / 4 + 16;
                    PS_CHECK(hipMalloc(reinterpret_cast<void **>(&d_filt), pair_cap * 4));
                }
                PS_RC(tracs_filter_recomb_pairs(a, d_rows, d_cols, d_d, (size_t)total, d_filt, nullptr));
                PS_CHECK(hipMemcpy(h32.data(), d_filt, (size_t)total * 4, hipMemcpyDeviceToHost));
                widen_append(res->filt, h32.data(), (size_t)total);
                lap(t_filter);
            }
        }
    }
    if (clock.on)
        std::fprintf(stderr, "[stage] dense panels (once-per-pack work + pair kernels) %.4f s\n[stage] COO extraction (device) %.4f s\n"
                             "[stage] COO D2H + widening to uint64 (%zu pairs) %.4f s\n[stage] recombination filter %.4f s\n",
                     t_dense, t_coo, res->rows.size(), t_pull, t_filter);
#undef PS_CHECK
#undef PS_RC
    // a Ctrl-C that arrived during the last panel / filter batch is not swallowed (the reference looks at its flag on every row)
    if (g_sigint) { cleanup(); delete res; set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }
    if (!filter) res->filt.assign(res->rows.size(), 0);      // filter off: `len` zeros (:452 via combine_vectors :31)
    cleanup();
    *out = res;
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
    tracs_alignment *a = nullptr;
    char *names = nullptr;
    size_t names_bytes = 0, n0 = 0;
    int rc = alignment_from_fasta_sites(fasta, n_fasta, &a, &names, &names_bytes, &n0, rule);
    if (rc) return rc;
    auto *res = new tracs_pairsnp_result();
    res->nseq = a->n; res->L = a->L;
    if (rule) res->source = std::move(rule->source);
    else res->source.rule_sites = a->L;
    const uint32_t min_sites = rule ? rule->min_sites : 0;
    { size_t o = 0; for (size_t i = 0; i < a->n; i++) { res->names.emplace_back(names + o); o += res->names.back().size() + 1; } }
    tracs_free(names);
    const size_t n = a->n;
    const size_t i_end = n_fasta == 1 ? n : n0;                     // pair ranges (src/pairsnp.hpp:348-360)
    const size_t j_start = n_fasta == 1 ? 0 : n0;
    const size_t n_lists = n_fasta == 1 ? n : n0;                   // two files: lists for the samples of file 0 only
    unsigned *d_dist = nullptr, *d_nn = nullptr, *d_out = nullptr;
    void *d_state = nullptr;
    long long *d_off = nullptr;
    auto cleanup = [&]() {
        void *p[] = {d_dist, d_nn, d_out, d_state, d_off};
        for (void *q : p) if (q) (void)hipFree(q);
        tracs_alignment_free(a);
    };
#define NN_CHECK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { cleanup(); delete res; set_error(std::string(#x ": ") + hipGetErrorString(e__)); return TRACS_E_HIP; } } while (0)
#define NN_RC(x) do { int r__ = (x); if (r__) { cleanup(); delete res; return r__; } } while (0)
#define NN_INTERRUPT() do { if (g_sigint) { cleanup(); delete res; set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; } } while (0)
    StageClock clock;
    size_t total = 0;
    if (n >= 2 && i_end > 0 && j_start < n) {
        NN_CHECK(hipMalloc(&d_state, tracs_knn_state_bytes(n_lists, k)));
        NN_RC(tracs_knn_init(d_state, n_lists, k, nullptr));
        // row panels bounded to ~1 GiB per dense matrix, as tracs_pairsnp / tracs_distance_run
        const size_t panel = std::max<size_t>(64, std::min<size_t>(i_end, (1ull << 28) / std::max<size_t>(n, 1)));
        NN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_dist), panel * n * 4));
        NN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_nn), panel * n * 4));
        for (size_t r0 = 0; r0 < i_end; r0 += panel) {
            NN_INTERRUPT();
            const size_t r1 = std::min(i_end, r0 + panel);
            unsigned *bd = d_dist - r0 * n, *bn = d_nn - r0 * n;     // addressed as base[i * ld + j] with i absolute
            NN_RC(tracs_pairsnp_dense_thr(a, r0, r1, j_start, bd, bn, n, dist, nullptr));
            if (min_sites) NN_RC(pairs_min_sites(bd, bn, n, n, r0, r1, j_start, dist, min_sites, nullptr));
            NN_RC(tracs_knn_update(bd, bn, n, n, r0, r1, j_start, dist, k, n_fasta == 1 ? 1 : 0, d_state, nullptr));
        }
        clock.mark("dense panels + selection");
        // rows, cols, d, nn, filt (and the filter's ordered pairs) in one block: one copy back
        const size_t cap = n_lists * (size_t)k;
        NN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_off), (n_lists + 1) * 8));
        NN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_out), cap * 4 * (filter ? 7 : 4)));
        unsigned *c_rows = d_out, *c_cols = d_out + cap, *c_d = d_out + 2 * cap, *c_n = d_out + 3 * cap;
        NN_RC(tracs_knn_emit(d_state, 0, n_lists, k, reinterpret_cast<int64_t *>(d_off), c_rows, c_cols, c_d, c_n, nullptr));
        long long tot = 0;
        NN_CHECK(hipMemcpy(&tot, d_off + n_lists, 8, hipMemcpyDeviceToHost));
        total = (size_t)tot;
        clock.mark("emit");
        if (filter && total) {
            NN_INTERRUPT();
            unsigned *c_f = d_out + 4 * cap, *c_lo = d_out + 5 * cap, *c_hi = d_out + 6 * cap;
            hipLaunchKernelGGL(knn_pair_order_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 65535)), dim3(256), 0, nullptr,
                               c_rows, c_cols, total, c_lo, c_hi);
            NN_CHECK(hipGetLastError());
            NN_RC(tracs_filter_recomb_pairs(a, c_lo, c_hi, c_d, total, c_f, nullptr));
            clock.mark("recombination filter");
        }
        if (total) {
            const size_t ncol = filter ? 5 : 4;
            std::vector<unsigned> h32(ncol * total);
            NN_CHECK(hipMemcpy2D(h32.data(), total * 4, d_out, cap * 4, total * 4, ncol, hipMemcpyDeviceToHost));
            widen_append(res->rows, h32.data(), total);
            widen_append(res->cols, h32.data() + total, total);
            widen_append(res->dist, h32.data() + 2 * total, total);
            widen_append(res->ncomp, h32.data() + 3 * total, total);
            if (filter) widen_append(res->filt, h32.data() + 4 * total, total);
            clock.mark("D2H + widening");
        }
    }
#undef NN_CHECK
#undef NN_RC
    if (g_sigint) { cleanup(); delete res; set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }
#undef NN_INTERRUPT
    if (!filter) res->filt.assign(res->rows.size(), 0);
    cleanup();
    *out = res;
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
    uint32_t *d_counts = nullptr;
    if (counts_host) {
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_counts), a->L * 6 * 4);
        if (e != hipSuccess) { (void)hipGetLastError(); set_error(std::string("hipMalloc(site census): ") + hipGetErrorString(e)); return TRACS_E_NOMEM; }
    }
    int rc = site_census(a, d_counts, differs_host, n_differs, nullptr);
    if (!rc && counts_host) {
        const hipError_t e = hipMemcpy(counts_host, d_counts, a->L * 6 * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { set_error(std::string("hipMemcpy(site census): ") + hipGetErrorString(e)); rc = TRACS_E_HIP; }
    }
    if (d_counts) (void)hipFree(d_counts);
    return rc;
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
    tracs_alignment *cut = nullptr;
    int rc = TRACS_OK;
    if (differing_only) {
        std::vector<uint64_t> differs((a->L + 63) / 64, 0);
        size_t nd = 0;
        if ((rc = site_census(a, nullptr, differs.data(), &nd, nullptr))) return rc;
        if (!nd) { set_error("no column differs among the samples"); return TRACS_E_ARG; }
        if ((rc = select_sites(const_cast<tracs_alignment *>(a), differs.data(), a->L, UINT32_MAX, &cut, nullptr, nullptr, nullptr, false))) return rc;
        a = cut;
    }
    const size_t L = a->L, stride = (L + 15) / 16 * 16, count = sample_end - sample_begin;
    const size_t batch = std::max<size_t>(1, std::min<size_t>(count, stride ? (256ull << 20) / stride : count));
    uint8_t *d_buf = nullptr, *h_buf = nullptr;
    auto done = [&](int r) {
        if (d_buf) (void)hipFree(d_buf);
        if (h_buf) (void)hipHostFree(h_buf);
        if (cut) tracs_alignment_free(cut);
        return r;
    };
#define WA_CHECK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { (void)hipGetLastError(); set_error(std::string(#x ": ") + hipGetErrorString(e__)); return done(TRACS_E_HIP); } } while (0)
    if (count && L) {
        WA_CHECK(hipMalloc(reinterpret_cast<void **>(&d_buf), batch * stride));
        WA_CHECK(hipHostMalloc(reinterpret_cast<void **>(&h_buf), batch * stride, hipHostMallocDefault));
    }
    if ((rc = tracs_write_fasta_rows(path, nullptr, nullptr, stride, 0, L, 0, n_threads, gzip_level))) return done(rc);     // truncate
    for (size_t s = sample_begin; s < sample_end; s += batch) {
        const size_t cnt = std::min(batch, sample_end - s);
        if (L) {
            if ((rc = unpack_rows(a, s, cnt, d_buf, stride, nullptr))) return done(rc);
            WA_CHECK(hipMemcpy(h_buf, d_buf, cnt * stride, hipMemcpyDeviceToHost));
        }
        if ((rc = tracs_write_fasta_rows(path, h->name_ptr.data() + s, h_buf, stride, cnt, L, 1, n_threads, gzip_level))) return done(rc);
    }
#undef WA_CHECK
    if (sites_written) *sites_written = L;
    return done(TRACS_OK);
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

// the date difference of every emitted pair, as tracs/transcluster.py:26-33 takes it: |t_i - t_j| / 31556952.0 with t = whole days in seconds
__global__ __launch_bounds__(256) void coo_delta_kernel(const unsigned *__restrict__ rows, const unsigned *__restrict__ cols, const int *__restrict__ days,
                                                        size_t n, double *__restrict__ out)
{
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (size_t)gridDim.x * 256) {
        const long long dd = (long long)days[rows[t]] - (long long)days[cols[t]];
        out[t] = (double)((dd < 0 ? -dd : dd) * 86400ll) / 31556952.0;
    }
}

int tracs_distance_run(tracs_distance *h, int dist, const int32_t *days, double lamb, double beta, double precision, double k_max,
                       const char *path, const char *ref, int filter, uint64_t *rows_written, uint64_t *n_pairs)
{
    if (rows_written) *rows_written = 0;
    if (n_pairs) *n_pairs = 0;
    if (!h || !h->a || !path || !ref) { set_error("tracs_distance_run: NULL argument"); return TRACS_E_ARG; }
    SigintScope sigint;
    tracs_alignment *a = h->a;
    const size_t n = a->n;
    const size_t i_end = h->n_fasta == 1 ? n : h->n0;               // pair ranges (:348-360)
    const size_t j_start = h->n_fasta == 1 ? 0 : h->n0;
    const bool with_dates = days != nullptr;
    // rows per device-to-host batch (TRACS_DISTANCE_BATCH_ROWS: diagnostics -- small batches in tests)
    static const size_t CH_MAX = [] { const char *e = std::getenv("TRACS_DISTANCE_BATCH_ROWS"); const long long v = e ? std::atoll(e) : 0; return v >= 16 ? (size_t)v : (size_t)1 << 22; }();
    // (never more than the pairs there can be: ten isolates do not pin a quarter of a gigabyte of host memory)
    const size_t CH = std::max<size_t>(64, std::min<size_t>(CH_MAX, (h->n_fasta == 1 ? h->a->n : h->n0) * h->a->n));
    unsigned *d_dist = nullptr, *d_nn = nullptr, *d_coo = nullptr;
    double *d_p = nullptr, *d_e = nullptr, *d_cp = nullptr;
    const bool dense_tc = with_dates && !filter;                   // --filter: the transmission model is driven by the FILTERED distance
                                                                    // (tracs/distance.py:183-193): per emitted pair, after the filter
    int *d_days = nullptr;
    long long *d_off = nullptr;
    char *pin[2] = {nullptr, nullptr};
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr}, ready = nullptr;
    tracs::DistanceRowWriter writer;
    auto cleanup = [&]() {
        void *p[] = {d_dist, d_nn, d_coo, d_p, d_e, d_cp, d_days, d_off};
        for (void *q : p) if (q) (void)hipFree(q);
        for (char *q : pin) if (q) (void)hipHostFree(q);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (ready) (void)hipEventDestroy(ready);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
    };
#define DR_CHECK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { cleanup(); set_error(std::string(#x ": ") + hipGetErrorString(e__)); return TRACS_E_HIP; } } while (0)
#define DR_RC(x) do { int r__ = (x); if (r__) { cleanup(); return r__; } } while (0)
    DR_RC(writer.open(path, h->name_ptr.data(), h->name_ptr.size(), ref));
    StageClock clock;
    double t_dense = 0.0, t_tc = 0.0, t_coo = 0.0, t_rows = 0.0;
    auto lap = [&](double &acc) {
        if (!clock.on) return;
        (void)hipDeviceSynchronize();
        const auto now = std::chrono::steady_clock::now();
        acc += std::chrono::duration<double>(now - clock.t).count();
        clock.t = now;
    };
    uint64_t pairs = 0;
    if (n >= 2 && i_end > 0) {
        // row panels bounded to ~1 GiB per uint32 matrix (2 GiB per f64 one)
        const size_t panel = std::max<size_t>(64, std::min<size_t>(i_end, (1ull << 28) / std::max<size_t>(n, 1)));
        DR_CHECK(hipMalloc(reinterpret_cast<void **>(&d_dist), panel * n * 4));
        DR_CHECK(hipMalloc(reinterpret_cast<void **>(&d_nn), panel * n * 4));
        DR_CHECK(hipMalloc(reinterpret_cast<void **>(&d_off), (panel + 1) * 8));
        if (dense_tc) {
            DR_CHECK(hipMalloc(reinterpret_cast<void **>(&d_p), panel * n * 8));
            DR_CHECK(hipMalloc(reinterpret_cast<void **>(&d_e), panel * n * 8));
        }
        if (with_dates) {
            DR_CHECK(hipMalloc(reinterpret_cast<void **>(&d_days), n * 4));
            DR_CHECK(hipMemcpy(d_days, days, n * 4, hipMemcpyHostToDevice));
        }
        // a batch on the host: four uint32 columns (five with --filter), then two f64 ones; two of them, so that one is formatted while the
        // next arrives
        const size_t n32 = filter ? 5 : 4;
        const size_t batch_bytes = CH * (n32 * 4 + (with_dates ? 16 : 0) + 4);
        for (auto &q : pin) DR_CHECK(hipHostMalloc(reinterpret_cast<void **>(&q), batch_bytes, hipHostMallocDefault));
        DR_CHECK(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
        for (auto &e : ev) DR_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        DR_CHECK(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
        std::vector<uint32_t> zeros;                                  // the filtered column without metadata: `len` zeros (:240-258)
        if (!with_dates) zeros.assign(CH, 0u);
        size_t cap = 0;
        for (size_t r0 = 0; r0 < i_end; r0 += panel) {
            if (g_sigint) { cleanup(); set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }
            const size_t r1 = std::min(i_end, r0 + panel);
            unsigned *bd = d_dist - r0 * n, *bn = d_nn - r0 * n;     // addressed as base[i * ld + j] with i absolute
            double *bp = dense_tc ? d_p - r0 * n : nullptr, *be = dense_tc ? d_e - r0 * n : nullptr;
            DR_RC(tracs_pairsnp_dense_thr(a, r0, r1, j_start, bd, bn, n, dist, nullptr));
            if (h->min_sites) DR_RC(pairs_min_sites(bd, bn, n, n, r0, r1, j_start, dist, h->min_sites, nullptr));
            lap(t_dense);
            if (dense_tc)
                DR_RC(tracs_trans_dist_dense(bd, n, n, r0, r1, j_start, dist, d_days, lamb, beta, precision, 1, bp, be, nullptr));
            lap(t_tc);
            DR_RC(tracs_coo_count(bd, n, n, r0, r1, j_start, dist, reinterpret_cast<int64_t *>(d_off), nullptr));
            long long total = 0;
            DR_CHECK(hipMemcpy(&total, d_off + (r1 - r0), 8, hipMemcpyDeviceToHost));
            if (total <= 0) continue;
            if ((size_t)total > cap) {
                if (d_coo) DR_CHECK(hipFree(d_coo));
                if (d_cp) DR_CHECK(hipFree(d_cp));
                d_coo = nullptr; d_cp = nullptr;
                cap = (size_t)total;
                DR_CHECK(hipMalloc(reinterpret_cast<void **>(&d_coo), cap * 4 * n32));
                if (with_dates) DR_CHECK(hipMalloc(reinterpret_cast<void **>(&d_cp), cap * (filter ? 24 : 16)));
            }
            unsigned *c_rows = d_coo, *c_cols = d_coo + cap, *c_d = d_coo + 2 * cap, *c_n = d_coo + 3 * cap, *c_f = filter ? d_coo + 4 * cap : nullptr;
            double *c_p = d_cp, *c_e = with_dates ? d_cp + cap : nullptr, *c_delta = (with_dates && filter) ? d_cp + 2 * cap : nullptr;
            DR_RC(tracs_coo_fill(bd, bn, n, n, r0, r1, j_start, dist, reinterpret_cast<int64_t *>(d_off), c_rows, c_cols, c_d, c_n, nullptr));
            if (dense_tc)
                DR_RC(tracs_coo_fill_f64(bd, n, n, r0, r1, j_start, dist, reinterpret_cast<int64_t *>(d_off), bp, be, c_p, c_e, nullptr));
            if (filter) {
                // the recombination filter on the emitted pairs (src/pairsnp.hpp:405-413), then -- with dates -- P(direct) and E(K) of the
                // filtered distances, pair by pair (tracs/distance.py:183-193 -> tracs/transcluster.py:8-41 -> trans_dist)
                DR_RC(tracs_filter_recomb_pairs(a, c_rows, c_cols, c_d, (size_t)total, c_f, nullptr));
                if (with_dates) {
                    hipLaunchKernelGGL(coo_delta_kernel, dim3((unsigned)std::min<size_t>(((size_t)total + 255) / 256, 65535)), dim3(256), 0, nullptr, c_rows, c_cols,
                                       d_days, (size_t)total, c_delta);
                    DR_RC(tracs_trans_dist_device(reinterpret_cast<const int32_t *>(c_f), c_delta, (size_t)total, lamb, beta, precision, 1, c_p, c_e, nullptr));
                }
                lap(t_tc);
            }
            DR_CHECK(hipEventRecord(ready, nullptr));
            DR_CHECK(hipStreamWaitEvent(copy_stream, ready, 0));
            lap(t_coo);
            const size_t nb = ((size_t)total + CH - 1) / CH;
            auto post = [&](size_t k) -> hipError_t {                 // batch k -> pinned set k % 2
                const size_t o = k * CH, cnt = std::min(CH, (size_t)total - o);
                char *dst = pin[k & 1];
                const unsigned *src32[5] = {c_rows, c_cols, c_d, c_n, c_f};
                for (size_t q = 0; q < n32; q++) {
                    const hipError_t e = hipMemcpyAsync(dst + (size_t)q * CH * 4, src32[q] + o, cnt * 4, hipMemcpyDeviceToHost, copy_stream);
                    if (e != hipSuccess) return e;
                }
                if (with_dates) {
                    const size_t f64_at = (CH * n32 * 4 + 7) / 8 * 8;
                    hipError_t e = hipMemcpyAsync(dst + f64_at, c_p + o, cnt * 8, hipMemcpyDeviceToHost, copy_stream);
                    if (e == hipSuccess) e = hipMemcpyAsync(dst + f64_at + CH * 8, c_e + o, cnt * 8, hipMemcpyDeviceToHost, copy_stream);
                    if (e != hipSuccess) return e;
                }
                return hipEventRecord(ev[k & 1], copy_stream);
            };
            DR_CHECK(post(0));
            for (size_t k = 0; k < nb; k++) {
                if (g_sigint) { (void)hipStreamSynchronize(copy_stream); cleanup(); set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }
                DR_CHECK(hipEventSynchronize(ev[k & 1]));
                if (k + 1 < nb) DR_CHECK(post(k + 1));
                const size_t cnt = std::min(CH, (size_t)total - k * CH);
                const char *src = pin[k & 1];
                const uint32_t *hr = reinterpret_cast<const uint32_t *>(src), *hc = hr + CH, *hd = hr + 2 * CH, *hn = hr + 3 * CH;
                const size_t f64_at = (CH * n32 * 4 + 7) / 8 * 8;
                const double *hp = reinterpret_cast<const double *>(src + f64_at), *he = hp + CH;
                // the filtered column: --filter: the filtered distances; else metadata on: a column of "NA" (:204), metadata off: zeros (:240-258)
                const uint32_t *hf = filter ? hr + 4 * CH : (with_dates ? nullptr : zeros.data());
                DR_RC(writer.append_u32(hr, hc, hd, hf, hn, days, with_dates ? hp : nullptr, with_dates ? he : nullptr,
                                        cnt, with_dates ? 1 : 0, with_dates ? k_max : -1.0));
            }
            pairs += (uint64_t)total;
            lap(t_rows);
        }
    }
    if (clock.on)
        std::fprintf(stderr, "[stage] dense panels (once-per-pack work + pair kernels) %.4f s\n[stage] transcluster on the panels (device) %.4f s\n"
                             "[stage] COO extraction (device) %.4f s\n[stage] rows: device -> host, format, write (%llu pairs) %.4f s\n",
                     t_dense, t_tc, t_coo, (unsigned long long)pairs, t_rows);
#undef DR_CHECK
#undef DR_RC
    cleanup();
    const int rc = writer.close();
    if (rows_written) *rows_written = writer.written();
    if (n_pairs) *n_pairs = pairs;
    if (g_sigint) { set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }
    return rc;
}

// `tracs distance --mst WEIGHT` for one alignment (include/tracs_hip.h): the panel loop of tracs_distance_run up to
// the COO of the panel's pairs within the threshold (with P and E(K), --filter's filtered distances and their P and E(K)), then
// tracs_msf_update_coo instead of the rows; after the last panel the forest is emitted and written through the same row writer.
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
    tracs_alignment *a = h->a;
    const size_t n = a->n;
    const size_t i_end = h->n_fasta == 1 ? n : h->n0;               // pair ranges (:348-360)
    const size_t j_start = h->n_fasta == 1 ? 0 : h->n0;
    const bool with_dates = days != nullptr;
    const bool dense_tc = with_dates && !filter;
    // rows per panel (TRACS_FOREST_PANEL_ROWS: diagnostics -- small panels in tests, so that the forest crosses panel boundaries)
    static const size_t PANEL_ROWS = [] { const char *e = std::getenv("TRACS_FOREST_PANEL_ROWS"); const long long v = e ? std::atoll(e) : 0; return v >= 1 ? (size_t)v : (size_t)0; }();
    unsigned *d_dist = nullptr, *d_nn = nullptr, *d_coo = nullptr;
    double *d_p = nullptr, *d_e = nullptr, *d_cp = nullptr;
    int *d_days = nullptr;
    long long *d_off = nullptr;
    void *d_state = nullptr;
    tracs::DistanceRowWriter writer;
    auto cleanup = [&]() {
        void *q[] = {d_dist, d_nn, d_coo, d_p, d_e, d_cp, d_days, d_off, d_state};
        for (void *x : q) if (x) (void)hipFree(x);
    };
#define MF_CHECK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { cleanup(); set_error(std::string(#x ": ") + hipGetErrorString(e__)); return TRACS_E_HIP; } } while (0)
#define MF_RC(x) do { int r__ = (x); if (r__) { cleanup(); return r__; } } while (0)
    MF_RC(writer.open(path, h->name_ptr.data(), h->name_ptr.size(), ref));
    StageClock clock;
    uint64_t eligible = 0;
    const double e_max = (with_dates && k_max >= 0.0) ? k_max : -1.0;
    if (n >= 2 && i_end > 0 && j_start < n) {
        const size_t panel = PANEL_ROWS ? std::min(PANEL_ROWS, i_end)
                                        : std::max<size_t>(64, std::min<size_t>(i_end, (1ull << 28) / std::max<size_t>(n, 1)));
        MF_CHECK(hipMalloc(&d_state, tracs_msf_state_bytes(n)));
        MF_RC(tracs_msf_init(d_state, n, nullptr));
        MF_CHECK(hipMalloc(reinterpret_cast<void **>(&d_dist), panel * n * 4));
        MF_CHECK(hipMalloc(reinterpret_cast<void **>(&d_nn), panel * n * 4));
        MF_CHECK(hipMalloc(reinterpret_cast<void **>(&d_off), (panel + 1) * 8));
        if (dense_tc) {
            MF_CHECK(hipMalloc(reinterpret_cast<void **>(&d_p), panel * n * 8));
            MF_CHECK(hipMalloc(reinterpret_cast<void **>(&d_e), panel * n * 8));
        }
        if (with_dates) {
            MF_CHECK(hipMalloc(reinterpret_cast<void **>(&d_days), n * 4));
            MF_CHECK(hipMemcpy(d_days, days, n * 4, hipMemcpyHostToDevice));
        }
        const size_t n32 = filter ? 5 : 4;
        size_t cap = 0;
        for (size_t r0 = 0; r0 < i_end; r0 += panel) {
            if (g_sigint) { cleanup(); set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }
            const size_t r1 = std::min(i_end, r0 + panel);
            unsigned *bd = d_dist - r0 * n, *bn = d_nn - r0 * n;     // addressed as base[i * ld + j] with i absolute
            double *bp = dense_tc ? d_p - r0 * n : nullptr, *be = dense_tc ? d_e - r0 * n : nullptr;
            MF_RC(tracs_pairsnp_dense_thr(a, r0, r1, j_start, bd, bn, n, dist, nullptr));
            if (h->min_sites) MF_RC(pairs_min_sites(bd, bn, n, n, r0, r1, j_start, dist, h->min_sites, nullptr));
            if (dense_tc)
                MF_RC(tracs_trans_dist_dense(bd, n, n, r0, r1, j_start, dist, d_days, lamb, beta, precision, 1, bp, be, nullptr));
            MF_RC(tracs_coo_count(bd, n, n, r0, r1, j_start, dist, reinterpret_cast<int64_t *>(d_off), nullptr));
            long long total = 0;
            MF_CHECK(hipMemcpy(&total, d_off + (r1 - r0), 8, hipMemcpyDeviceToHost));
            if (total <= 0) continue;
            if ((size_t)total > cap) {
                if (d_coo) MF_CHECK(hipFree(d_coo));
                if (d_cp) MF_CHECK(hipFree(d_cp));
                d_coo = nullptr; d_cp = nullptr;
                cap = (size_t)total;
                MF_CHECK(hipMalloc(reinterpret_cast<void **>(&d_coo), cap * 4 * n32));
                if (with_dates) MF_CHECK(hipMalloc(reinterpret_cast<void **>(&d_cp), cap * (filter ? 24 : 16)));
            }
            unsigned *c_rows = d_coo, *c_cols = d_coo + cap, *c_d = d_coo + 2 * cap, *c_n = d_coo + 3 * cap, *c_f = filter ? d_coo + 4 * cap : nullptr;
            double *c_p = d_cp, *c_e = with_dates ? d_cp + cap : nullptr, *c_delta = (with_dates && filter) ? d_cp + 2 * cap : nullptr;
            MF_RC(tracs_coo_fill(bd, bn, n, n, r0, r1, j_start, dist, reinterpret_cast<int64_t *>(d_off), c_rows, c_cols, c_d, c_n, nullptr));
            if (dense_tc)
                MF_RC(tracs_coo_fill_f64(bd, n, n, r0, r1, j_start, dist, reinterpret_cast<int64_t *>(d_off), bp, be, c_p, c_e, nullptr));
            if (filter) {
                MF_RC(tracs_filter_recomb_pairs(a, c_rows, c_cols, c_d, (size_t)total, c_f, nullptr));
                if (with_dates) {
                    hipLaunchKernelGGL(coo_delta_kernel, dim3((unsigned)std::min<size_t>(((size_t)total + 255) / 256, 65535)), dim3(256), 0, nullptr, c_rows, c_cols,
                                       d_days, (size_t)total, c_delta);
                    MF_RC(tracs_trans_dist_device(reinterpret_cast<const int32_t *>(c_f), c_delta, (size_t)total, lamb, beta, precision, 1, c_p, c_e, nullptr));
                }
            }
            // the weight the cluster step reads: column 3 (d), 6 (filtered d), 4 (P), 5 (E(K)); -K drops pairs with E(K) above it or NaN
            const void *wv = weight == 0 ? (const void *)c_d : weight == 1 ? (const void *)c_f : weight == 2 ? (const void *)c_p : (const void *)c_e;
            uint64_t taken = 0;
            MF_RC(tracs_msf_update_coo(d_state, n, (size_t)total, c_rows, c_cols, wv, weight >= 2 ? 1 : 0, e_max >= 0.0 ? c_e : nullptr, e_max,
                                       c_d, c_n, c_f, c_p, c_e, &taken, nullptr));
            eligible += taken;
        }
        clock.mark("dense panels + transcluster + forest updates");
        size_t nf = 0;
        MF_RC(tracs_msf_emit(d_state, n, &nf, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        if (nf) {
            // the forest's rows: rows, cols, d, nn, filt (uint32), P, E(K) (f64) -- < n of them
            if (d_coo) MF_CHECK(hipFree(d_coo));
            if (d_cp) MF_CHECK(hipFree(d_cp));
            d_coo = nullptr; d_cp = nullptr;
            MF_CHECK(hipMalloc(reinterpret_cast<void **>(&d_coo), nf * 4 * 5));
            MF_CHECK(hipMalloc(reinterpret_cast<void **>(&d_cp), nf * 16));
            MF_RC(tracs_msf_emit(d_state, n, &nf, d_coo, d_coo + nf, d_coo + 2 * nf, d_coo + 3 * nf, d_coo + 4 * nf, d_cp, d_cp + nf, nullptr));
            std::vector<uint32_t> h32(nf * 5);
            std::vector<double> h64(nf * 2);
            MF_CHECK(hipMemcpy(h32.data(), d_coo, nf * 20, hipMemcpyDeviceToHost));
            MF_CHECK(hipMemcpy(h64.data(), d_cp, nf * 16, hipMemcpyDeviceToHost));
            const uint32_t *hr = h32.data(), *hc = hr + nf, *hd = hr + 2 * nf, *hn = hr + 3 * nf, *hf = hr + 4 * nf;
            // the filtered column as the full run writes it: --filter: the filtered distances; else metadata on: "NA", off: zeros (:240-258)
            MF_RC(writer.append_u32(hr, hc, hd, filter ? hf : (with_dates ? nullptr : hf), hn, days, with_dates ? h64.data() : nullptr,
                                    with_dates ? h64.data() + nf : nullptr, nf, with_dates ? 1 : 0, -1.0));
        }
        clock.mark("forest rows: emit, device -> host, format, write");
    }
#undef MF_CHECK
#undef MF_RC
    cleanup();
    const int rc = writer.close();
    if (rows_written) *rows_written = writer.written();
    if (n_eligible) *n_eligible = eligible;
    if (g_sigint) { set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }
    return rc;
}

// `tracs distance --ancestors WEIGHT` for one alignment (include/tracs_hip.h): the panel loop of tracs_distance_forest
// with tracs_anc_update_coo instead of the forest update; after the last panel the links are emitted and written through the same row
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
    tracs_alignment *a = h->a;
    const size_t n = a->n;
    const size_t i_end = h->n_fasta == 1 ? n : h->n0;               // pair ranges (:348-360)
    const size_t j_start = h->n_fasta == 1 ? 0 : h->n0;
    const bool dense_tc = !filter;
    // rows per panel (TRACS_FOREST_PANEL_ROWS: diagnostics -- small panels in tests, as tracs_distance_forest)
    static const size_t PANEL_ROWS = [] { const char *e = std::getenv("TRACS_FOREST_PANEL_ROWS"); const long long v = e ? std::atoll(e) : 0; return v >= 1 ? (size_t)v : (size_t)0; }();
    unsigned *d_dist = nullptr, *d_nn = nullptr, *d_coo = nullptr, *d_tree = nullptr;
    double *d_p = nullptr, *d_e = nullptr, *d_cp = nullptr;
    int *d_days = nullptr;
    long long *d_off = nullptr;
    void *d_state = nullptr;
    tracs::DistanceRowWriter writer;
    auto cleanup = [&]() {
        void *q[] = {d_dist, d_nn, d_coo, d_tree, d_p, d_e, d_cp, d_days, d_off, d_state};
        for (void *x : q) if (x) (void)hipFree(x);
    };
#define AN_CHECK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { cleanup(); set_error(std::string(#x ": ") + hipGetErrorString(e__)); return TRACS_E_HIP; } } while (0)
#define AN_RC(x) do { int r__ = (x); if (r__) { cleanup(); return r__; } } while (0)
    AN_RC(writer.open(path, h->name_ptr.data(), h->name_ptr.size(), ref));
    StageClock clock;
    uint64_t eligible = 0;
    const double e_max = k_max >= 0.0 ? k_max : -1.0;
    std::vector<uint32_t> tree(n * 3);                              // parent, root, generation
    for (size_t s = 0; s < n; s++) { tree[s] = 0xFFFFFFFFu; tree[n + s] = (uint32_t)s; tree[2 * n + s] = 0; }      // (no pair at all: every sample a root)
    if (n >= 2 && i_end > 0 && j_start < n) {
        const size_t panel = PANEL_ROWS ? std::min(PANEL_ROWS, i_end)
                                        : std::max<size_t>(64, std::min<size_t>(i_end, (1ull << 28) / std::max<size_t>(n, 1)));
        AN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_days), n * 4));
        AN_CHECK(hipMemcpy(d_days, days, n * 4, hipMemcpyHostToDevice));
        AN_CHECK(hipMalloc(&d_state, tracs_anc_state_bytes(n)));
        AN_RC(tracs_anc_init(d_state, n, d_days, nullptr));
        AN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_dist), panel * n * 4));
        AN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_nn), panel * n * 4));
        AN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_off), (panel + 1) * 8));
        if (dense_tc) {
            AN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_p), panel * n * 8));
            AN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_e), panel * n * 8));
        }
        const size_t n32 = filter ? 5 : 4;
        size_t cap = 0;
        for (size_t r0 = 0; r0 < i_end; r0 += panel) {
            if (g_sigint) { cleanup(); set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }
            const size_t r1 = std::min(i_end, r0 + panel);
            unsigned *bd = d_dist - r0 * n, *bn = d_nn - r0 * n;     // addressed as base[i * ld + j] with i absolute
            double *bp = dense_tc ? d_p - r0 * n : nullptr, *be = dense_tc ? d_e - r0 * n : nullptr;
            AN_RC(tracs_pairsnp_dense_thr(a, r0, r1, j_start, bd, bn, n, dist, nullptr));
            if (h->min_sites) AN_RC(pairs_min_sites(bd, bn, n, n, r0, r1, j_start, dist, h->min_sites, nullptr));
            if (dense_tc)
                AN_RC(tracs_trans_dist_dense(bd, n, n, r0, r1, j_start, dist, d_days, lamb, beta, precision, 1, bp, be, nullptr));
            AN_RC(tracs_coo_count(bd, n, n, r0, r1, j_start, dist, reinterpret_cast<int64_t *>(d_off), nullptr));
            long long total = 0;
            AN_CHECK(hipMemcpy(&total, d_off + (r1 - r0), 8, hipMemcpyDeviceToHost));
            if (total <= 0) continue;
            if ((size_t)total > cap) {
                if (d_coo) AN_CHECK(hipFree(d_coo));
                if (d_cp) AN_CHECK(hipFree(d_cp));
                d_coo = nullptr; d_cp = nullptr;
                cap = (size_t)total;
                AN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_coo), cap * 4 * n32));
                AN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_cp), cap * (filter ? 24 : 16)));
            }
            unsigned *c_rows = d_coo, *c_cols = d_coo + cap, *c_d = d_coo + 2 * cap, *c_n = d_coo + 3 * cap, *c_f = filter ? d_coo + 4 * cap : nullptr;
            double *c_p = d_cp, *c_e = d_cp + cap, *c_delta = filter ? d_cp + 2 * cap : nullptr;
            AN_RC(tracs_coo_fill(bd, bn, n, n, r0, r1, j_start, dist, reinterpret_cast<int64_t *>(d_off), c_rows, c_cols, c_d, c_n, nullptr));
            if (dense_tc)
                AN_RC(tracs_coo_fill_f64(bd, n, n, r0, r1, j_start, dist, reinterpret_cast<int64_t *>(d_off), bp, be, c_p, c_e, nullptr));
            if (filter) {
                AN_RC(tracs_filter_recomb_pairs(a, c_rows, c_cols, c_d, (size_t)total, c_f, nullptr));
                hipLaunchKernelGGL(coo_delta_kernel, dim3((unsigned)std::min<size_t>(((size_t)total + 255) / 256, 65535)), dim3(256), 0, nullptr, c_rows, c_cols,
                                   d_days, (size_t)total, c_delta);
                AN_RC(tracs_trans_dist_device(reinterpret_cast<const int32_t *>(c_f), c_delta, (size_t)total, lamb, beta, precision, 1, c_p, c_e, nullptr));
            }
            // the value a source is chosen by: d, filtered d and E(K) ascending, P(direct) descending; -K drops pairs with E(K) above it or NaN
            const void *wv = weight == 0 ? (const void *)c_d : weight == 1 ? (const void *)c_f : weight == 2 ? (const void *)c_p : (const void *)c_e;
            uint64_t taken = 0;
            AN_RC(tracs_anc_update_coo(d_state, n, (size_t)total, c_rows, c_cols, wv, weight == 2 ? 2 : weight == 3 ? 1 : 0,
                                       e_max >= 0.0 ? c_e : nullptr, e_max, c_d, c_n, c_f, c_p, c_e, &taken, nullptr));
            eligible += taken;
        }
        clock.mark("dense panels + transcluster + ancestor updates");
        size_t nl = 0;
        AN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_tree), n * 12));
        AN_RC(tracs_anc_emit(d_state, n, &nl, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_tree, d_tree + n, d_tree + 2 * n, nullptr));
        AN_CHECK(hipMemcpy(tree.data(), d_tree, n * 12, hipMemcpyDeviceToHost));
        if (nl) {
            // the links' rows: rows, cols, d, nn, filt (uint32), P, E(K) (f64) -- < n of them
            if (d_coo) AN_CHECK(hipFree(d_coo));
            if (d_cp) AN_CHECK(hipFree(d_cp));
            d_coo = nullptr; d_cp = nullptr;
            AN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_coo), nl * 4 * 5));
            AN_CHECK(hipMalloc(reinterpret_cast<void **>(&d_cp), nl * 16));
            AN_RC(tracs_anc_emit(d_state, n, &nl, d_coo, d_coo + nl, d_coo + 2 * nl, d_coo + 3 * nl, d_coo + 4 * nl, d_cp, d_cp + nl, nullptr, nullptr,
                                 nullptr, nullptr));
            std::vector<uint32_t> h32(nl * 5);
            std::vector<double> h64(nl * 2);
            AN_CHECK(hipMemcpy(h32.data(), d_coo, nl * 20, hipMemcpyDeviceToHost));
            AN_CHECK(hipMemcpy(h64.data(), d_cp, nl * 16, hipMemcpyDeviceToHost));
            const uint32_t *hr = h32.data(), *hc = hr + nl, *hd = hr + 2 * nl, *hn = hr + 3 * nl, *hf = hr + 4 * nl;
            // the filtered column as the full run writes it with metadata: --filter: the filtered distances; else "NA" (:204)
            AN_RC(writer.append_u32(hr, hc, hd, filter ? hf : nullptr, hn, days, h64.data(), h64.data() + nl, nl, 1, -1.0));
        }
        clock.mark("ancestor rows: emit, device -> host, format, write");
    }
#undef AN_CHECK
#undef AN_RC
    cleanup();
    int rc = writer.close();
    if (rows_written) *rows_written = writer.written();
    if (n_eligible) *n_eligible = eligible;
    if (g_sigint) { set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }
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

// `tracs distance --histogram` for one alignment (include/tracs_hip.h): the panel loop of tracs_distance_run with
// tracs_hist_update on each dense panel instead of the rows; with --filter the panel's pairs within the threshold are extracted and
// filtered as tracs_distance_run does, and a second state counts their filtered distances.  What crosses to the host is the
// non-empty bins.
int tracs_distance_histogram(tracs_distance *h, int dist, int filter, const int32_t *group, const char *path, const char *ref,
                             uint64_t *n_eligible, uint64_t *rows_written)
{
    if (rows_written) *rows_written = 0;
    if (n_eligible) *n_eligible = 0;
    if (!h || !h->a || !path || !ref) { set_error("tracs_distance_histogram: NULL argument"); return TRACS_E_ARG; }
    if (dist < 0) { set_error("tracs_distance_histogram: dist must not be negative"); return TRACS_E_ARG; }
    SigintScope sigint;
    tracs_alignment *a = h->a;
    const size_t n = a->n;
    const size_t i_end = h->n_fasta == 1 ? n : h->n0;               // pair ranges (:348-360)
    const size_t j_start = h->n_fasta == 1 ? 0 : h->n0;
    const size_t n_bins = std::min<size_t>(a->L, (size_t)dist) + 1;  // d <= L and d <= dist: no eligible value falls outside
    // rows per panel (TRACS_FOREST_PANEL_ROWS: diagnostics -- small panels in tests, as tracs_distance_forest)
    static const size_t PANEL_ROWS = [] { const char *e = std::getenv("TRACS_FOREST_PANEL_ROWS"); const long long v = e ? std::atoll(e) : 0; return v >= 1 ? (size_t)v : (size_t)0; }();
    unsigned *d_dist = nullptr, *d_nn = nullptr, *d_coo = nullptr, *d_val = nullptr;
    int *d_group = nullptr;
    long long *d_off = nullptr;
    void *d_state[2] = {nullptr, nullptr};
    uint64_t *d_cnt = nullptr;
    auto cleanup = [&]() {
        void *q[] = {d_dist, d_nn, d_coo, d_val, d_group, d_off, d_state[0], d_state[1], d_cnt};
        for (void *x : q) if (x) (void)hipFree(x);
    };
#define HG_CHECK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { cleanup(); set_error(std::string(#x ": ") + hipGetErrorString(e__)); return TRACS_E_HIP; } } while (0)
#define HG_RC(x) do { int r__ = (x); if (r__) { cleanup(); return r__; } } while (0)
    FILE *fp = std::fopen(path, "ab");
    if (!fp) { set_error(std::string("cannot open ") + path + " for appending"); return TRACS_E_OPEN; }
    struct Closer { FILE *&f; ~Closer() { if (f) std::fclose(f); } } closer{fp};
    StageClock clock;
    uint64_t eligible = 0, written = 0;
    if (n >= 2 && i_end > 0 && j_start < n) {
        const size_t panel = PANEL_ROWS ? std::min(PANEL_ROWS, i_end)
                                        : std::max<size_t>(64, std::min<size_t>(i_end, (1ull << 28) / std::max<size_t>(n, 1)));
        const int n_states = filter ? 2 : 1;
        for (int s = 0; s < n_states; s++) {
            HG_CHECK(hipMalloc(&d_state[s], tracs_hist_state_bytes(n_bins)));
            HG_RC(tracs_hist_init(d_state[s], n_bins, nullptr));
        }
        HG_CHECK(hipMalloc(reinterpret_cast<void **>(&d_dist), panel * n * 4));
        HG_CHECK(hipMalloc(reinterpret_cast<void **>(&d_nn), panel * n * 4));
        if (group) {
            HG_CHECK(hipMalloc(reinterpret_cast<void **>(&d_group), n * 4));
            HG_CHECK(hipMemcpy(d_group, group, n * 4, hipMemcpyHostToDevice));
        }
        if (filter) HG_CHECK(hipMalloc(reinterpret_cast<void **>(&d_off), (panel + 1) * 8));
        size_t cap = 0;
        for (size_t r0 = 0; r0 < i_end; r0 += panel) {
            if (g_sigint) { cleanup(); set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }
            const size_t r1 = std::min(i_end, r0 + panel);
            unsigned *bd = d_dist - r0 * n, *bn = d_nn - r0 * n;     // addressed as base[i * ld + j] with i absolute
            HG_RC(tracs_pairsnp_dense_thr(a, r0, r1, j_start, bd, bn, n, dist, nullptr));
            if (h->min_sites) HG_RC(pairs_min_sites(bd, bn, n, n, r0, r1, j_start, dist, h->min_sites, nullptr));
            HG_RC(tracs_hist_update(bd, n, n, r0, r1, j_start, dist, d_group, d_state[0], n_bins, nullptr));
            if (!filter) continue;
            // the filtered distances of the panel's eligible pairs (src/pairsnp.hpp:405-413), as tracs_distance_run takes them
            HG_RC(tracs_coo_count(bd, n, n, r0, r1, j_start, dist, reinterpret_cast<int64_t *>(d_off), nullptr));
            long long total = 0;
            HG_CHECK(hipMemcpy(&total, d_off + (r1 - r0), 8, hipMemcpyDeviceToHost));
            if (total <= 0) continue;
            if ((size_t)total > cap) {
                if (d_coo) { void *old = d_coo; d_coo = nullptr; HG_CHECK(hipFree(old)); }
                cap = (size_t)total;
                HG_CHECK(hipMalloc(reinterpret_cast<void **>(&d_coo), cap * 4 * 5));
            }
            unsigned *c_rows = d_coo, *c_cols = d_coo + cap, *c_d = d_coo + 2 * cap, *c_n = d_coo + 3 * cap, *c_f = d_coo + 4 * cap;
            HG_RC(tracs_coo_fill(bd, bn, n, n, r0, r1, j_start, dist, reinterpret_cast<int64_t *>(d_off), c_rows, c_cols, c_d, c_n, nullptr));
            HG_RC(tracs_filter_recomb_pairs(a, c_rows, c_cols, c_d, (size_t)total, c_f, nullptr));
            HG_RC(tracs_hist_update_coo(c_rows, c_cols, c_f, (size_t)total, d_group, d_state[1], n_bins, nullptr));
        }
        clock.mark("dense panels + histogram updates");
        static const char *const column[2] = {"snp", "filter"};
        std::string text;
        for (int s = 0; s < n_states; s++) {
            size_t nr = 0;
            HG_RC(tracs_hist_emit(d_state[s], n_bins, &nr, nullptr, nullptr, nullptr, nullptr, nullptr));
            if (!nr) continue;
            if (d_val) { void *old = d_val; d_val = nullptr; HG_CHECK(hipFree(old)); }
            if (d_cnt) { void *old = d_cnt; d_cnt = nullptr; HG_CHECK(hipFree(old)); }
            HG_CHECK(hipMalloc(reinterpret_cast<void **>(&d_val), nr * 4));
            HG_CHECK(hipMalloc(reinterpret_cast<void **>(&d_cnt), nr * 8 * 3));
            HG_RC(tracs_hist_emit(d_state[s], n_bins, &nr, d_val, d_cnt, d_cnt + nr, d_cnt + 2 * nr, nullptr));
            std::vector<uint32_t> hv(nr);
            std::vector<uint64_t> hc(nr * 3);
            HG_CHECK(hipMemcpy(hv.data(), d_val, nr * 4, hipMemcpyDeviceToHost));
            HG_CHECK(hipMemcpy(hc.data(), d_cnt, nr * 24, hipMemcpyDeviceToHost));
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
            cleanup();
            set_error(std::string("write to ") + path + " failed");
            return TRACS_E_OPEN;
        }
        clock.mark("histogram rows: emit, device -> host, format, write");
    }
#undef HG_CHECK
#undef HG_RC
    cleanup();
    const int rc_close = std::fclose(fp);
    fp = nullptr;
    if (rc_close != 0) { set_error(std::string("write to ") + path + " failed"); return TRACS_E_OPEN; }
    if (rows_written) *rows_written = written;
    if (n_eligible) *n_eligible = eligible;
    if (g_sigint) { set_error("Interrupted by user!"); return TRACS_E_INTERRUPTED; }
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
