// test_dynamic_bitset.cpp -- every member of the stand-in boost/dynamic_bitset.hpp against a naive std::vector<bool>.
// A stand-alone program (its own main; never loaded into Python): tests/test_pairsnp_ref.py compiles it with
// -fsanitize=address,undefined and runs it.  Exit status 0 and the line "bitset ok" mean every check held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <boost/dynamic_bitset.hpp>

typedef boost::dynamic_bitset<> bits;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()                                              // splitmix64
{
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int failures = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) {                                                         \
            failures++;                                                        \
            std::printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond);        \
            std::printf(__VA_ARGS__);                                          \
            std::printf("\n");                                                 \
        }                                                                      \
    } while (0)

static size_t naive_count(const std::vector<bool> &v)
{
    size_t c = 0;
    for (size_t i = 0; i < v.size(); i++) c += v[i];
    return c;
}

static size_t naive_from(const std::vector<bool> &v, size_t p)     // first set position >= p, npos when none
{
    for (size_t i = p; i < v.size(); i++)
        if (v[i]) return i;
    return bits::npos;
}

static void same(const bits &b, const std::vector<bool> &v, const char *what, size_t n, int fill)
{
    CHECK(b.size() == v.size(), "%s n=%zu fill=%d", what, n, fill);
    CHECK(b.count() == naive_count(v), "%s n=%zu fill=%d count %zu", what, n, fill, b.count());
    for (size_t i = 0; i < v.size(); i++) CHECK(b[i] == v[i], "%s n=%zu fill=%d bit %zu", what, n, fill, i);
    CHECK(b.find_first() == naive_from(v, 0), "%s n=%zu fill=%d find_first", what, n, fill);
    for (size_t i = 0; i < v.size(); i++)                          // find_next from every position, set or not, the last one included
        CHECK(b.find_next(i) == naive_from(v, i + 1), "%s n=%zu fill=%d find_next(%zu)", what, n, fill, i);
    // the walk the reference does: an int loop variable compared with npos
    size_t walked = 0;
    for (int i = b.find_first(); i != bits::npos; i = b.find_next(i)) walked++;
    CHECK(walked == naive_count(v), "%s n=%zu fill=%d walk", what, n, fill);
}

static void fill_random(bits &b, std::vector<bool> &v, int fill)   // fill: 0 none, 1 sparse, 2 half, 3 dense, 4 all
{
    for (size_t i = 0; i < v.size(); i++) {
        const uint64_t r = rnd() % 100;
        const bool on = fill == 0 ? false : fill == 1 ? r < 3 : fill == 2 ? r < 50 : fill == 3 ? r < 97 : true;
        v[i] = on;
        if (on) b[i] = 1;                                          // assignment through the proxy, as load_seqs does
    }
}

int main()
{
    static_assert(bits::npos == static_cast<size_t>(-1), "npos");
    const size_t sizes[] = {0, 1, 63, 64, 65, 128, 1000};
    for (size_t n : sizes)
        for (int fill = 0; fill <= 4; fill++) {
            bits a(n), b(n);
            std::vector<bool> va(n), vb(n);
            same(a, va, "fresh", n, fill);                          // (n): all clear
            fill_random(a, va, fill);
            fill_random(b, vb, 2);
            same(a, va, "assigned", n, fill);
            if (n) {                                                // clearing through the proxy; the last position
                a[n - 1] = 0; va[n - 1] = false;
                same(a, va, "last cleared", n, fill);
                a[n - 1] = 1; va[n - 1] = true;
                same(a, va, "last set", n, fill);
                CHECK(a.find_next(n - 1) == bits::npos, "find_next(last) n=%zu", n);
            }
            bits c(a);                                              // copy, then change the copy alone
            same(c, va, "copy", n, fill);
            if (n) {
                c[0] = !va[0];
                CHECK(a[0] == va[0], "copy is deep n=%zu", n);
            }
            std::vector<bool> vand(n), vor(n), vflip(n);
            for (size_t i = 0; i < n; i++) {
                vand[i] = va[i] && vb[i];
                vor[i] = va[i] || vb[i];
                vflip[i] = !va[i];
            }
            bits d(n);
            d = a & b;                                              // assignment from a temporary, as the pair loop does
            same(d, vand, "and", n, fill);
            bits e(a);
            e |= b;
            same(e, vor, "or", n, fill);
            e |= a & b;                                             // |= of a temporary changes nothing here
            same(e, vor, "or of and", n, fill);
            bits f(a);
            f.flip();                                               // nothing beyond size(): count and the finds see it at once
            same(f, vflip, "flip", n, fill);
            CHECK(f.count() + a.count() == n, "flip count n=%zu", n);
            f.flip();
            same(f, va, "flip twice", n, fill);
            same(a, va, "operand untouched", n, fill);
            same(b, vb, "operand untouched", n, fill);
        }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("bitset ok\n");
    return 0;
}
