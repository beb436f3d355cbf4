// boost/dynamic_bitset.hpp -- a STAND-IN, not Boost.  TEST INFRASTRUCTURE ONLY.
//
// Written for this project from the documented interface of a run-time sized bitset, so that the
// reference's src/pairsnp.hpp compiles unmodified from where it lies (oracle/Makefile puts
// -Ioracle/boost_standin ahead of every other include path).  It provides exactly the members that
// header uses: (n), copy, operator[] read and assignment, &, |=, flip, count, size, find_first,
// find_next and npos.  Each is checked against a naive std::vector<bool> by
// oracle/boost_standin/test_dynamic_bitset.cpp (run under ASan + UBSan by tests/test_pairsnp_ref.py).
//
// Invariant: no bit is set at or beyond size() in the last word -- flip() restores it, so count(),
// find_first() and find_next() never see a bit that is not there.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

namespace boost {

template <typename Block = unsigned long, typename Allocator = std::allocator<Block>>
class dynamic_bitset {
    static_assert(sizeof(Block) == 8, "the stand-in keeps 64-bit words");

  public:
    typedef std::size_t size_type;
    static const size_type npos = static_cast<size_type>(-1);      // the reference compares an int loop variable with it

    class reference {
        Block &w_;
        Block m_;

      public:
        reference(Block &w, Block m) : w_(w), m_(m) {}
        reference &operator=(bool v)
        {
            if (v) w_ |= m_; else w_ &= ~m_;
            return *this;
        }
        reference &operator=(const reference &o) { return *this = static_cast<bool>(o); }
        operator bool() const { return (w_ & m_) != 0; }
    };

    explicit dynamic_bitset(size_type n = 0) : n_(n), w_((n + 63) / 64, Block(0)) {}

    size_type size() const { return n_; }

    reference operator[](size_type i) { return reference(w_[i >> 6], Block(1) << (i & 63)); }
    bool operator[](size_type i) const { return (w_[i >> 6] >> (i & 63)) & 1; }

    dynamic_bitset &operator|=(const dynamic_bitset &o)             // sizes must be equal, as the real one requires
    {
        for (size_type i = 0; i < w_.size(); i++) w_[i] |= o.w_[i];
        return *this;
    }
    friend dynamic_bitset operator&(const dynamic_bitset &a, const dynamic_bitset &b)
    {
        dynamic_bitset r(a);
        for (size_type i = 0; i < r.w_.size(); i++) r.w_[i] &= b.w_[i];
        return r;
    }

    dynamic_bitset &flip()
    {
        for (size_type i = 0; i < w_.size(); i++) w_[i] = ~w_[i];
        if (n_ & 63) w_.back() &= (Block(1) << (n_ & 63)) - 1;       // nothing set beyond size()
        return *this;
    }

    size_type count() const
    {
        size_type c = 0;
        for (size_type i = 0; i < w_.size(); i++) c += static_cast<size_type>(__builtin_popcountll(w_[i]));
        return c;
    }

    size_type find_first() const { return from(0); }
    // the first set bit after p; npos when there is none, p is the last position, or p is outside the set
    size_type find_next(size_type p) const { return (p >= n_ || p + 1 >= n_) ? npos : from(p + 1); }

  private:
    size_type from(size_type p) const                               // first set bit at or after p (p < size() or size() == 0)
    {
        size_type i = p >> 6;
        if (i >= w_.size()) return npos;
        Block w = w_[i] & (~Block(0) << (p & 63));
        while (true) {
            if (w) return i * 64 + static_cast<size_type>(__builtin_ctzll(w));
            if (++i == w_.size()) return npos;
            w = w_[i];
        }
    }

    size_type n_;
    std::vector<Block, Allocator> w_;
};

template <typename B, typename A>
const typename dynamic_bitset<B, A>::size_type dynamic_bitset<B, A>::npos;

}  // namespace boost
