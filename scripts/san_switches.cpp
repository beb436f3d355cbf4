// san_switches.cpp -- the accessors of csrc/switches.h under AddressSanitizer + UBSan on the host: every kind on values that are unset,
// empty, 0, 1, negative, no number and beyond INT_MAX, and the two lifetimes pinned with setenv between reads.  No GPU, no HIP, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer scripts/san_switches.cpp -lpthread -o /tmp/san_switches \
//       && ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1 /tmp/san_switches
//
// (scripts/sanitize_host.sh runs it beside san_alloc.cpp.)
#include "../tracs_amd/csrc/switches.h"

#include <climits>
#include <cmath>
#include <cstdio>

#define EXPECT(x) do { if (!(x)) { std::fprintf(stderr, "san_switches: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

using namespace tracs;

static void put(sw::Id id, const char *value)
{
    if (value) setenv(sw::table[id].name, value, 1);
    else unsetenv(sw::table[id].name);
}

int main()
{
    for (int id = 0; id < sw::count; id++) unsetenv(sw::table[id].name);
    EXPECT(sizeof(sw::table) / sizeof(sw::table[0]) == sw::count && !std::strcmp(sw::table[sw::TRACS_KSPLIT].name, "TRACS_KSPLIT"));

    // ---- every kind, on rows that are read from the environment every time ------------------------------------------------------------
    const sw::Id I = sw::TRACS_KSPLIT, S = sw::TRACS_NN_SEGMENT_MB, Z = sw::TRACS_FILTER_LISTS, T = sw::TRACS_FILTER_LONG, F = sw::TRACS_STAGE_TRACE;
    EXPECT(sw::table[I].life == sw::Life::every && sw::table[S].life == sw::Life::every && sw::table[Z].life == sw::Life::every &&
           sw::table[T].life == sw::Life::every && sw::table[F].life == sw::Life::every);
    // unset: the caller's value, and nothing is set, zero or text
    EXPECT(sw::integer(I, -7) == -7 && sw::integer(I, 5LL) == 5LL && sw::size(S, 256) == 256 && !sw::is_zero(Z) && !sw::text(T) && !sw::is_set(F));
    // empty: set, and the number 0 (as atoi, strtoull give); not "off", whose first character must be '0'
    put(I, ""); put(S, ""); put(Z, ""); put(T, ""); put(F, "");
    EXPECT(sw::integer(I, -7) == 0 && sw::size(S, 256) == 0 && !sw::is_zero(Z) && sw::text(T) && !*sw::text(T) && sw::is_set(F) && sw::is_set(I));
    put(I, "0"); put(S, "0"); put(Z, "0"); put(T, "0"); put(F, "0");
    EXPECT(sw::integer(I, -7) == 0 && sw::size(S, 256) == 0 && sw::is_zero(Z) && !std::strcmp(sw::text(T), "0") && sw::is_set(F));      // a flag set to 0 is set
    put(I, "1"); put(S, "1"); put(Z, "1"); put(T, "seq");
    EXPECT(sw::integer(I, -7) == 1 && sw::size(S, 256) == 1 && !sw::is_zero(Z) && sw::text(T)[0] == 's');
    put(I, " -12x"); put(S, "-1"); put(Z, "-0"); put(Z, "0no");
    EXPECT(sw::integer(I, -7) == -12 && sw::size(S, 256) == ULLONG_MAX && sw::is_zero(Z));                      // strtoull's "-1"; the first character alone
    put(I, "seq"); put(S, "many"); put(Z, "off");
    EXPECT(sw::integer(I, -7) == 0 && sw::size(S, 256) == 0 && !sw::is_zero(Z));
    // beyond INT_MAX: the nearest value of the type asked for, never an overflow
    put(I, "4294967297"); put(S, "4294967297");
    EXPECT(sw::integer(I, -7) == INT_MAX && sw::integer(I, 0L) == 4294967297L && sw::integer(I, 0LL) == 4294967297LL && sw::size(S, 0) == 4294967297ull);
    put(I, "-99999999999999999999999"); put(S, "99999999999999999999999");
    EXPECT(sw::integer(I, -7) == INT_MIN && sw::integer(I, 0LL) == LLONG_MIN && sw::size(S, 0) == ULLONG_MAX);
    put(I, nullptr); put(S, nullptr); put(Z, nullptr); put(T, nullptr); put(F, nullptr);
    EXPECT(sw::integer(I, -7) == -7 && sw::size(S, 9) == 9 && !sw::is_zero(Z) && !sw::text(T) && !sw::is_set(F));                      // `every` follows the environment

    // ---- fractions: every such row is read once, so each shows one value -----------------------------------------------------------------
    EXPECT(sw::table[sw::TRACS_PACK_ARENA].life == sw::Life::once && sw::table[sw::TRACS_NN_LIST_K].life == sw::Life::once);
    put(sw::TRACS_PACK_ARENA, "0.25"); put(sw::TRACS_MINOR_BUDGET_DIV, "-abc"); put(sw::TRACS_LIST_CAP, "1e999");
    EXPECT(sw::real(sw::TRACS_PACK_ARENA, 0.3) == 0.25 && sw::real(sw::TRACS_MINOR_BUDGET_DIV, 2000.0) == 0.0 && std::isinf(sw::real(sw::TRACS_LIST_CAP, -1.0)) &&
           sw::real(sw::TRACS_NN_LIST_K, 6e-6) == 6e-6);
    put(sw::TRACS_PACK_ARENA, "0"); put(sw::TRACS_NN_LIST_K, "1");
    EXPECT(sw::real(sw::TRACS_PACK_ARENA, 0.3) == 0.25 && sw::real(sw::TRACS_NN_LIST_K, 6e-6) == 6e-6);                                   // kept: set or not

    // ---- `once`: the first read's value whatever the environment does later, whichever accessor asks ----------------------------------
    EXPECT(sw::table[sw::TRACS_MFMA].life == sw::Life::once && sw::table[sw::TRACS_FORCE_GENERAL].life == sw::Life::once);
    put(sw::TRACS_MFMA, "0"); put(sw::TRACS_FORCE_GENERAL, "0");
    EXPECT(sw::integer(sw::TRACS_MFMA, -1) == 0 && sw::is_set(sw::TRACS_FORCE_GENERAL) && !sw::is_set(sw::TRACS_TILE_VARIANT));
    put(sw::TRACS_MFMA, "1"); put(sw::TRACS_FORCE_GENERAL, nullptr); put(sw::TRACS_TILE_VARIANT, "2");
    EXPECT(sw::integer(sw::TRACS_MFMA, -1) == 0 && sw::is_set(sw::TRACS_FORCE_GENERAL) && !sw::is_set(sw::TRACS_TILE_VARIANT) && sw::integer(sw::TRACS_TILE_VARIANT, -1) == -1);
    put(sw::TRACS_MFMA, nullptr);
    EXPECT(sw::integer(sw::TRACS_MFMA, -1) == 0 && sw::is_set(sw::TRACS_MFMA));
    put(sw::TRACS_MFMA_TILE, "3x2");
    const char *tile = sw::text(sw::TRACS_MFMA_TILE);
    put(sw::TRACS_MFMA_TILE, "2x2");
    EXPECT(!std::strcmp(tile, "3x2") && sw::text(sw::TRACS_MFMA_TILE) == tile);                                                             // the kept copy, not the environment's
    // ... and an `every` row in the same breath
    put(I, "3");
    EXPECT(sw::integer(I, 0) == 3);
    put(I, "4");
    EXPECT(sw::integer(I, 0) == 4);
    std::puts("san_switches ok");
    return 0;
}
