// san_alloc.cpp -- the owners of csrc/common.h and the allocation path of csrc/alloc_path.h under AddressSanitizer + UBSan on the host,
// against stub HIP calls (plain malloc / free, linked into this program only).  No GPU, no Python.
//
//   hipcc -std=c++17 -O1 -g -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scripts/san_alloc.cpp -o /tmp/san_alloc && ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1 /tmp/san_alloc
//
// (scripts/sanitize_host.sh runs it beside the host-only sources' driver.)
#include "../tracs_amd/csrc/alloc_path.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

// ---- the stubs: this program's definitions take precedence over the HIP runtime's ----------------------------------------------------
static long g_stub_live = 0;
extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { *p = bytes ? std::malloc(bytes) : nullptr; g_stub_live += *p != nullptr; return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { *p = bytes ? std::malloc(bytes) : nullptr; g_stub_live += *p != nullptr; return hipSuccess; }
hipError_t hipFree(void *p) { g_stub_live -= p != nullptr; std::free(p); return hipSuccess; }
hipError_t hipHostFree(void *p) { g_stub_live -= p != nullptr; std::free(p); return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "stub error"; }
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { std::memcpy(dst, src, bytes); return hipSuccess; }
}

static std::string g_message;
void tracs::set_error(const std::string &msg) { g_message = msg; }

#define EXPECT(x) do { if (!(x)) { std::fprintf(stderr, "san_alloc: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

using namespace tracs;

static bool stats_are(uint64_t blocks, uint64_t bytes, uint64_t pinned)
{
    uint64_t s[4];
    alloc_stats(s);
    return s[0] == blocks && s[1] == bytes && s[2] == pinned && g_stub_live == (long)(blocks + pinned);
}

int main()
{
    uint64_t s[4];
    alloc_stats(s);
    EXPECT(s[0] == 0 && s[1] == 0 && s[2] == 0 && s[3] == 0);
    {
        DeviceArray<uint32_t> a, b;
        PinnedArray<double> h;
        EXPECT(a.alloc(100, "a") == TRACS_OK && b.alloc(7, "b") == TRACS_OK && h.alloc(3, "h") == TRACS_OK);
        a.get()[99] = 1u; b.get()[6] = 2u; h.get()[2] = 3.0;
        EXPECT(stats_are(2, 428, 1));
        DeviceArray<uint32_t> c(std::move(a));                               // move: a is empty, c holds its block
        EXPECT(!a.get() && c.get()[99] == 1u && c.count() == 100 && stats_are(2, 428, 1));
        c = std::move(b);                                                    // move-assign onto a held buffer: c's block goes
        EXPECT(!b.get() && c.get()[6] == 2u && stats_are(1, 28, 1));
        c = std::move(c);                                                    // onto itself: nothing happens
        EXPECT(c.get()[6] == 2u && stats_are(1, 28, 1));
        DeviceBuffer raw;
        EXPECT(raw.grow(64, "raw") == TRACS_OK);
        void *first = raw.ptr;
        EXPECT(raw.grow(32, "raw") == TRACS_OK && raw.ptr == first && raw.bytes == 64);          // large enough: kept
        EXPECT(raw.grow(65, "raw") == TRACS_OK && raw.bytes == 65 && stats_are(2, 93, 1));        // too small: replaced, an exact fit
        const char text[] = "upload";
        EXPECT(raw.upload(text, sizeof text, "text") == TRACS_OK && std::strcmp(raw.as<char>(), "upload") == 0);
        raw.release();
        raw.release();                                                       // twice: the second finds nothing
        EXPECT(!raw.ptr && !raw.bytes && stats_are(1, 28, 1));
        uint32_t *mine = c.detach();                                         // the block is the caller's
        EXPECT(!c.get() && mine[6] == 2u && stats_are(1, 28, 1));
        device_free(mine);
        device_free(nullptr);
        pinned_free(nullptr);
        EXPECT(stats_are(0, 0, 1));
        DeviceArray<uint8_t> none;
        EXPECT(none.alloc(0, "nothing") == TRACS_OK && !none.get() && stats_are(0, 0, 1));       // 0 bytes: NULL, not counted
        // the one-shot failure count: the third allocation from now, device or pinned, then off again
        alloc_stats(s);
        fail_alloc(3);
        DeviceArray<int> x, y, z;
        PinnedArray<int> p;
        EXPECT(x.alloc(1, "x") == TRACS_OK && p.alloc(1, "p") == TRACS_OK);
        g_message.clear();
        EXPECT(y.alloc(5, "why") == TRACS_E_NOMEM && !y.get() && g_message == "hipMalloc(why, 20 bytes): out of memory");
        EXPECT(z.alloc(1, "z") == TRACS_OK);
        alloc_stats(s);
        EXPECT(s[3] == 4 && s[0] == 2 && s[1] == 8 && s[2] == 2);            // the failed one counts as an allocation made
        alloc_stats(s);
        EXPECT(s[3] == 0);                                                   // reading resets the fourth
        fail_alloc(1);
        g_message = "kept";
        EXPECT(!y.try_alloc(5) && !y.get() && g_message.empty());            // try_alloc failing: no block, the error slot clear
        EXPECT(y.try_alloc(5) && y.count() == 5);
        fail_alloc(1);
        EXPECT(p.alloc(2, "pin") == TRACS_E_NOMEM && !p.get() && g_message == "hipHostMalloc(pin, 8 bytes): out of memory");
        alloc_stats(s);
        EXPECT(s[2] == 1);                                                   // alloc() let go of what p held before it failed
        fail_alloc(2);
        fail_alloc(0);                                                       // 0 turns it off
        EXPECT(p.alloc(2, "pin") == TRACS_OK && x.alloc(2, "x") == TRACS_OK);
    }
    EXPECT(stats_are(0, 0, 0));                                             // every owner gave its block back
    std::puts("san_alloc ok");
    return 0;
}
