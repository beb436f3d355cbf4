// boost/math/distributions/binomial.hpp -- a STAND-IN, not Boost.  TEST INFRASTRUCTURE ONLY.
//
// Written for this project so that the reference's src/pairsnp.hpp compiles unmodified from where it
// lies (oracle/Makefile: -Ioracle/boost_standin first).  It provides the two names that header uses,
// boost::math::binomial_distribution<>(n, p) and boost::math::cdf(dist, k), and nothing else.
//
// cdf(dist, k) = P(X <= k), X ~ Binomial(n, p), as the regularised finite sum, NOT Boost's incomplete
// beta: the numerics are ours.  What the reference's control flow does with the value is the
// reference's; the value itself is held to the definition at 50 digits by tests/test_pairsnp_ref.py
// (|(1 - cdf) - tail| <= 1e-9 * 0.05 / d on the cells the fixtures decide).
//
// Method: the sum is taken on the side of k that does not hold the mode, from its largest term
// outwards -- every term positive, each a ratio times the one before.  Above the mode the upper tail T
// is summed and 1 - T returned (so 1 - cdf gives T back to a rounding of cdf); at or below it the
// lower sum itself.  The largest term C(n, j) p^j (1 - p)^(n - j) is a product of its factors with
// the binary exponent kept apart (no underflow at n = 10 001), (1 - p)^(n - j) through log1p.
#pragma once
#include <cmath>
#include <stdexcept>

namespace boost {
namespace math {

template <class RealType = double>
class binomial_distribution {
  public:
    binomial_distribution(RealType n, RealType p) : n_(n), p_(p)
    {
        if (!(n >= 0) || !(p >= 0 && p <= 1) || n != std::floor(n))
            throw std::domain_error("binomial_distribution stand-in: n must be a whole number >= 0 and p within [0, 1]");
    }
    RealType trials() const { return n_; }
    RealType success_fraction() const { return p_; }

  private:
    RealType n_, p_;
};

namespace standin_detail {

// C(n, j) p^j (1 - p)^(n - j) for 0 < p < 1
inline double binomial_term(long n, long j, double p)
{
    double v = 1.0;
    long e = 0;
    int ex;
    const long m = j < n - j ? j : n - j;                       // C(n, j) = C(n, m)
    for (long i = 1; i <= m; i++) {
        v *= static_cast<double>(n - m + i) / static_cast<double>(i);
        v = std::frexp(v, &ex);
        e += ex;
    }
    for (long i = 0; i < j; i++) {
        v *= p;
        v = std::frexp(v, &ex);
        e += ex;
    }
    const double t = static_cast<double>(n - j) * std::log1p(-p) / 0.693147180559945309417232121458;   // log2 of (1 - p)^(n - j)
    const double ti = std::floor(t);
    v *= std::exp2(t - ti);
    if (static_cast<double>(e) + ti < -1070.0) return 0.0;
    return std::ldexp(v, static_cast<int>(e + static_cast<long>(ti)));
}

inline double binomial_cdf(long n, double p, long k)
{
    if (k >= n) return 1.0;
    if (p == 0.0) return 1.0;
    if (p == 1.0) return 0.0;
    const double q = 1.0 - p;
    if (static_cast<double>(k + 1) > (static_cast<double>(n) + 1.0) * p) {
        // k + 1 is past the mode: the upper tail's terms fall from j = k + 1 on
        const double first = binomial_term(n, k + 1, p);
        double term = 1.0, sum = 1.0;
        for (long j = k + 1; j < n; j++) {
            term *= static_cast<double>(n - j) / static_cast<double>(j + 1) * p / q;
            sum += term;
            if (term < 1e-20 * sum) break;
        }
        return 1.0 - first * sum;
    }
    // k is at or below the mode: the lower sum's terms fall from j = k down
    const double first = binomial_term(n, k, p);
    double term = 1.0, sum = 1.0;
    for (long j = k; j > 0; j--) {
        term *= static_cast<double>(j) / static_cast<double>(n - j + 1) * q / p;
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return first * sum;
}

}  // namespace standin_detail

template <class RealType>
inline RealType cdf(const binomial_distribution<RealType> &dist, const RealType &k)
{
    if (!(k >= 0 && k <= dist.trials()))
        throw std::domain_error("binomial cdf stand-in: k must lie within [0, n]");
    return static_cast<RealType>(standin_detail::binomial_cdf(static_cast<long>(dist.trials()), static_cast<double>(dist.success_fraction()),
                                                              static_cast<long>(std::floor(k))));
}

// the reference passes an int where the distribution's RealType is double
template <class RealType, class K>
inline RealType cdf(const binomial_distribution<RealType> &dist, const K &k)
{
    return cdf(dist, static_cast<RealType>(k));
}

}  // namespace math
}  // namespace boost
