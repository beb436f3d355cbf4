// switches.h -- the library's run-time switches: one table, one row per environment variable, and the accessors
// that read it.  Host only, nothing from HIP.  No other file under csrc/ calls getenv (tests/test_switches.py).  Clamps, rounding,
// ranges and the words of a text switch are the policy of the site that reads, not of the parser here.
#ifndef TRACS_SWITCHES_H
#define TRACS_SWITCHES_H

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>

namespace tracs {
namespace sw {

// what the value is, and its accessor: flag -- set or not, "=0" is set (is_set, which serves every other kind too); zero_off -- off when
// the first character is '0' (is_zero); integer, real, size -- a number (integer, real, size: the second argument is the value when the
// variable is not set); text -- a word matched at the site (text)
enum class Kind { flag, zero_off, integer, real, size, text };
// once: read at the first use in the process and kept, whatever the environment does later (tests start a child process);
// every: read from the environment at every use -- once per call or per pack, where the site stands
enum class Life { once, every };

// clang-format off
#define TRACS_SWITCHES(X) \
    X(TRACS_MFMA,                 integer,  once,  "0: every alignment uses the VALU tile kernel") \
    X(TRACS_TILE_VARIANT,         integer,  once,  "VALU tile shape 0..3; set at all: no matrix cores") \
    X(TRACS_FORCE_GENERAL,        flag,     once,  "never use the consensus encoding") \
    X(TRACS_GENERAL_MFMA,         integer,  once,  "general alignments: 0 never, 1 always the one-hot matrix-core kernel + sparse correction") \
    X(TRACS_THR_ONE_PASS,         flag,     once,  "thresholded runs: a single pass") \
    X(TRACS_KSPLIT,               integer,  every, "workgroups per tile along the alignment") \
    X(TRACS_THR_PREFIX,           integer,  every, "thresholded runs: prefix length in groups") \
    X(TRACS_SUPERTILE,            text,     once,  "<rows>x<cols>: tiles per supertile of the tile schedule") \
    X(TRACS_PACK_ARENA,           real,     once,  "fraction of the planes reserved with them as the pack's arena; 0: none") \
    X(TRACS_MFMA_TILE,            text,     once,  "workgroup shape of the matrix-core kernels") \
    X(TRACS_COUNT_TILE,           text,     once,  "workgroup tile of the counting pass") \
    X(TRACS_SITE_CLASSES,         integer,  once,  "0 never, 1 always cut the alignment into site classes") \
    X(TRACS_MINORITY,             integer,  once,  "0: site classes without the minority lists") \
    X(TRACS_MINOR_BUDGET_DIV,     real,     once,  "minority sites: k (cN + k) <= n^2 / x") \
    X(TRACS_NN_LISTS,             integer,  once,  "0: never take N co-occurrences from lists") \
    X(TRACS_NN_LIST_K,            real,     once,  "N lists while cN x lines <= k n^2") \
    X(TRACS_QLINE_DWORDS,         integer,  once,  "32 or 64: width of the p lists' q lines") \
    X(TRACS_COUNT_IN_PLACE,       integer,  once,  "counting pass: 0 never, 1 always the stored N plane in place") \
    X(TRACS_LIST_CAP,             real,     once,  "a smaller cap on the lists, in entries of 4 bytes") \
    X(TRACS_NW_GRAM,              integer,  every, "site classes: 0 never, 1 always the second form") \
    X(TRACS_NW_ROWS,              integer,  every, "second form: N x listed terms 0 from the U pass, 1 from the rows of the site-major N matrix") \
    X(TRACS_CLASSIFY_THREADS,     integer,  every, "workgroup size of the classifying kernel") \
    X(TRACS_CLASSES_TRACE,        flag,     once,  "once-per-pack stages and the filter index's build on stderr") \
    X(TRACS_ROW_LISTS,            integer,  once,  "rows' N sites for the list walk: 0 always bitmaps, 1 always slots") \
    X(TRACS_NN_SEGMENT_MB,        size,     every, "MiB of list lines per segment of the list walk; 0: one segment") \
    X(TRACS_TC_GRID,              integer,  once,  "0: transcluster on dense blocks through the hash route") \
    X(TRACS_FILTER_LISTS,         zero_off, every, "filter_recomb: always the scan of the planes") \
    X(TRACS_FILTER_TABLE,         zero_off, every, "filter_recomb: the binomial tail summed per SNP, not the per-d threshold rows") \
    X(TRACS_FILTER_CAP,           integer,  every, "filter_recomb: LDS capacity per list, in entries") \
    X(TRACS_FILTER_KERNEL,        integer,  every, "filter_recomb: 1 the binary-search kernel") \
    X(TRACS_FILTER_LONG,          text,     every, "filter_recomb: seq, the sequential long-list kernel") \
    X(TRACS_FILTER_SCAN_MAXPOS,   size,     every, "filter_recomb: SNP sites per batch of the scan") \
    X(TRACS_FILTER_LANES_MIN,     size,     every, "filter_recomb, scan route: pair-per-lane extraction from this many pairs on") \
    X(TRACS_PAIR_SITES_LANES_MIN, size,     every, "pair-sites: pair-per-lane count and fill from this many pairs on") \
    X(TRACS_PAIR_SITES_BATCH,     size,     every, "pair-sites: entries per batch of tracs_distance_pair_sites") \
    X(TRACS_FITCH_SLAB_GROUPS,    size,     every, "tree changes: groups of 128 sites per slab of the node-set buffer") \
    X(TRACS_FITCH_MATRIX_CHUNKS,  size,     every, "tree filter: chunks of 2 048 sites per range of the [chunk][edge] matrix") \
    X(TRACS_FITCH_BATCH,          size,     every, "tree changes: entries per batch of tracs_distance_tree_changes") \
    X(TRACS_MASK_RANGE,           size,     every, "tree iterate: (entry, leaf) cells per launch of mask_cells_kernel") \
    X(TRACS_HIST_GRID,            integer,  once,  "tracs_hist_update: workgroups per launch at most") \
    X(TRACS_DISTANCE_BATCH_ROWS,  integer,  every, "tracs distance: rows per device-to-host batch of the device-resident route") \
    X(TRACS_FOREST_PANEL_ROWS,    integer,  every, "host entry points: rows per dense panel of the panel walk") \
    X(TRACS_STAGE_TRACE,          flag,     every, "host entry-point stages on stderr") \
    X(TRACS_SERIAL_FASTA,         flag,     every, "always the serial kseq restatement")
// clang-format on

#define TRACS_SW_ID(name, kind, life, effect) name,
enum Id { TRACS_SWITCHES(TRACS_SW_ID) count };
#undef TRACS_SW_ID
struct Row { const char *name; Kind kind; Life life; const char *effect; };
#define TRACS_SW_ROW(name, kind, life, effect) { #name, Kind::kind, Life::life, effect },
inline constexpr Row table[] = { TRACS_SWITCHES(TRACS_SW_ROW) };
#undef TRACS_SW_ROW

// the variable's value, or NULL when it is not set (a `once` row: in a copy that is never freed, so that no destructor runs under a late caller)
inline const char *text(Id id)
{
    const Row &r = table[id];
    if (r.life == Life::every) return std::getenv(r.name);
    static struct { std::once_flag read; const char *value; } kept[count];
    std::call_once(kept[id].read, [&] {
        const char *e = std::getenv(r.name);
        kept[id].value = e ? std::strcpy(static_cast<char *>(std::malloc(std::strlen(e) + 1)), e) : nullptr;
    });
    return kept[id].value;
}
inline bool is_set(Id id) { return text(id) != nullptr; }
inline bool is_zero(Id id) { const char *e = text(id); return e && e[0] == '0'; }
// (what atoi / atol / atoll give wherever they are defined; beyond T's range, T's nearest value)
template <class T> inline T integer(Id id, T unset)
{
    const char *e = text(id);
    return e ? (T)std::clamp<long long>(std::strtoll(e, nullptr, 10), std::numeric_limits<T>::min(), std::numeric_limits<T>::max()) : unset;
}
inline double real(Id id, double unset) { const char *e = text(id); return e ? std::strtod(e, nullptr) : unset; }
// (strtoull: "-1" is the largest value, as it has been at every such site)
inline unsigned long long size(Id id, unsigned long long unset) { const char *e = text(id); return e ? std::strtoull(e, nullptr, 10) : unset; }

}   // namespace sw
}   // namespace tracs
#endif
