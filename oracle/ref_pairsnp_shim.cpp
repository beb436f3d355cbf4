// ref_pairsnp_shim.cpp -- the REFERENCE's src/pairsnp.hpp, compiled unmodified from where it lies
// (-I$(REF)/src) into oracle/_ref/_tracs_ref_pairsnp*.so.
//
// TEST INFRASTRUCTURE ONLY (see oracle/tracs_oracle.c header).  No reference source is copied: this
// file only #includes the reference header and gives it a Python face.  The two Boost headers it asks
// for are our own stand-ins (oracle/boost_standin, first on the include path): load_seqs, the pair
// loop, the emission rule and order, range_count and filter_recomb's control flow are the
// reference's; the bitset's members and the binomial CDF's numerics are ours.
//
// pybind11 comes first: the reference header calls PyErr_CheckSignals and leans on <vector> / <tuple>
// having been pulled in, as its python_bindings.cpp does.  Call ref_pairsnp with n_threads = 1: the
// reference polls Python's signals inside its OpenMP loop, which only the thread holding the GIL may do.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <algorithm>
#include <csignal>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "pairsnp.hpp"

namespace py = pybind11;

// 1 where the pair agrees, 0 at the listed sites: what filter_recomb expects before its own flip
static boost::dynamic_bitset<> match_bits(size_t L, const std::vector<size_t> &positions)
{
    boost::dynamic_bitset<> res(L);
    res.flip();
    for (size_t p : positions) {
        if (p >= L) throw std::out_of_range("position beyond the alignment");
        res[p] = 0;
    }
    return res;
}

#ifndef REF_PAIRSNP_MODULE_NAME
#define REF_PAIRSNP_MODULE_NAME _tracs_ref_pairsnp
#endif
PYBIND11_MODULE(REF_PAIRSNP_MODULE_NAME, m)
{
    m.doc() = "reference TRACS pairsnp.hpp compiled in place over stand-in bitset / binomial headers (oracle/_ref)";
    m.def("ref_pairsnp", [](const std::vector<std::string> &fastas, int n_threads, int dist, bool filter) {
        auto before = std::signal(SIGINT, SIG_DFL);                // pairsnp() installs its own SIGINT handler: put the caller's back
        try {
            auto out = pairsnp(fastas, n_threads, dist, filter);
            std::signal(SIGINT, before);
            return out;
        } catch (...) {
            std::signal(SIGINT, before);
            throw;
        }
    }, py::arg("fastas"), py::arg("n_threads"), py::arg("dist"), py::arg("filter"));
    m.def("ref_filter_recomb_positions", [](size_t L, const std::vector<size_t> &positions) {
        return filter_recomb(match_bits(L, positions));
    }, py::arg("L"), py::arg("positions"));
    // (length, count) of the set bits within [start, end); the reference leaves length unset when there is none: we return 0 then
    m.def("ref_range_count", [](size_t L, const std::vector<size_t> &positions, size_t start, size_t end) {
        boost::dynamic_bitset<> snps = match_bits(L, positions);
        snps.flip();
        std::pair<size_t, size_t> r = range_count(snps, start, end);
        if (r.second == 0) r.first = 0;
        return r;
    }, py::arg("L"), py::arg("positions"), py::arg("start"), py::arg("end"));
    m.def("ref_cached_binomial_cdf", [](int n, double p, int k) { return cached_binomial_cdf(n, p, k); },
          py::arg("n"), py::arg("p"), py::arg("k"));
}
