// alloc_path.h -- the allocation path of libtracs_hip.so: the definitions of common.h's device_alloc / device_free / pinned_alloc /
// pinned_free, the only callers of hipMalloc, hipHostMalloc, hipFree and hipHostFree in csrc/.  Included once, by capi.hip (beside
// the workspace); scripts/san_alloc.cpp includes it against stub HIP calls for the host sanitizer run.
//
// State: four counters, the one-shot failure count and -- so that a free knows how many bytes leave -- the size of every live device
// block, all under one mutex.  None of it is on a hot path: the dense call's timed loop allocates nothing.
#pragma once
#include "common.h"

#include <mutex>
#include <unordered_map>

namespace tracs {

struct AllocPath {
    std::mutex mu;
    uint64_t device_blocks = 0, device_bytes = 0, pinned_blocks = 0, allocs = 0;     // live, live, live, since the last reading
    long fail_in = 0;                       // tracs_debug_fail_alloc: the allocation that fails, counted down (0: off)
    std::unordered_map<void *, size_t> size;
};
static AllocPath g_alloc;

// counts the allocation; true: it is the one tracs_debug_fail_alloc named
static bool alloc_begin()
{
    std::lock_guard<std::mutex> lock(g_alloc.mu);
    g_alloc.allocs++;
    return g_alloc.fail_in > 0 && --g_alloc.fail_in == 0;
}
static int alloc_end(bool pinned, bool injected, hipError_t e, size_t bytes, const char *what, void **out)
{
    if (e != hipSuccess) {
        if (!injected) (void)hipGetLastError();
        *out = nullptr;
        set_error(std::string(pinned ? "hipHostMalloc(" : "hipMalloc(") + what + ", " + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
        return TRACS_E_NOMEM;
    }
    std::lock_guard<std::mutex> lock(g_alloc.mu);
    if (!*out) return TRACS_OK;               // (0 bytes: HIP may hand out NULL, which the frees pass over)
    if (pinned) g_alloc.pinned_blocks++;
    else { g_alloc.device_blocks++; g_alloc.device_bytes += bytes; g_alloc.size[*out] = bytes; }
    return TRACS_OK;
}

int device_alloc(size_t bytes, const char *what, void **out)
{
    *out = nullptr;
    const bool injected = alloc_begin();
    return alloc_end(false, injected, injected ? hipErrorOutOfMemory : hipMalloc(out, bytes), bytes, what, out);
}
int pinned_alloc(size_t bytes, const char *what, void **out)
{
    *out = nullptr;
    const bool injected = alloc_begin();
    return alloc_end(true, injected, injected ? hipErrorOutOfMemory : hipHostMalloc(out, bytes, hipHostMallocDefault), bytes, what, out);
}

bool device_try_alloc(size_t bytes, void **out)
{
    if (device_alloc(bytes, "optional block", out) == TRACS_OK) return true;
    set_error("");
    return false;
}

void device_free(void *p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> lock(g_alloc.mu);
        const auto it = g_alloc.size.find(p);
        if (it != g_alloc.size.end()) { g_alloc.device_blocks--; g_alloc.device_bytes -= it->second; g_alloc.size.erase(it); }
    }
    (void)hipFree(p);
}

void pinned_free(void *p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> lock(g_alloc.mu);
        g_alloc.pinned_blocks--;
    }
    (void)hipHostFree(p);
}

// out[4] <- live device blocks, live device bytes, live pinned blocks, allocations since the last reading (which this one resets)
static void alloc_stats(uint64_t *out)
{
    std::lock_guard<std::mutex> lock(g_alloc.mu);
    out[0] = g_alloc.device_blocks; out[1] = g_alloc.device_bytes; out[2] = g_alloc.pinned_blocks; out[3] = g_alloc.allocs;
    g_alloc.allocs = 0;
}
// the nth allocation from now (1-based, device or pinned) fails as out of memory without reaching HIP; one shot, 0 turns it off
static void fail_alloc(long nth)
{
    std::lock_guard<std::mutex> lock(g_alloc.mu);
    g_alloc.fail_in = nth > 0 ? nth : 0;
}

}  // namespace tracs
