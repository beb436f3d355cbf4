// common.h -- shared host-side helpers of libtracs_hip.so (error slot, the owners of device and pinned memory, layout constants).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tracs_hip.h"
#include "switches.h"

namespace tracs {

void set_error(const std::string &msg);

#define TRACS_HIP_CHECK(expr)                                                                   \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess) {                                                                \
            ::tracs::set_error(std::string(#expr) + ": " + hipGetErrorString(e__));             \
            return TRACS_E_HIP;                                                                 \
        }                                                                                       \
    } while (0)

// ---- device and pinned memory ----------------------------------------------------------
// Every byte the library owns comes from these four (alloc_path.h, part of capi.hip): nothing else in csrc/ calls hipMalloc,
// hipHostMalloc, hipFree or hipHostFree.  A failed allocation sets the error slot to "hipMalloc(<what>, <bytes> bytes): <HIP's
// text>" ("hipHostMalloc(..." for pinned memory), leaves *out NULL and HIP's last error clear, and returns TRACS_E_NOMEM.  The frees
// take NULL.  tracs_debug_alloc_stats / tracs_debug_fail_alloc read and steer the path's counters.
int device_alloc(size_t bytes, const char *what, void **out);
void device_free(void *p);
int pinned_alloc(size_t bytes, const char *what, void **out);
void pinned_free(void *p);
// an optional block: not getting it is not an error.  false leaves *out NULL and the error slot clear (as workspace_try)
bool device_try_alloc(size_t bytes, void **out);

// Owners: what a call allocates is freed when it returns, on every path, and what a structure holds goes with it.  Move-only.
// alloc() replaces what is held, grow() only when it is too small (an exact fit: the pair buffers never hold slack).  The destructor
// relies on hipFree waiting for the device; an owner is declared BEFORE whatever still uses it at scope exit (a stream that copies
// into it, see capi.hip's CopyLane), so that it is destroyed after it.
template <bool kPinned> struct OwnedBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;
    OwnedBuffer() = default;
    OwnedBuffer(OwnedBuffer &&o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
    OwnedBuffer &operator=(OwnedBuffer &&o) noexcept
    {
        if (this != &o) { release(); ptr = o.ptr; bytes = o.bytes; o.ptr = nullptr; o.bytes = 0; }
        return *this;
    }
    ~OwnedBuffer() { release(); }
    void release()
    {
        if (kPinned) pinned_free(ptr); else device_free(ptr);
        ptr = nullptr; bytes = 0;
    }
    int alloc(size_t want, const char *what)
    {
        release();
        const int rc = kPinned ? pinned_alloc(want, what, &ptr) : device_alloc(want, what, &ptr);
        if (rc == TRACS_OK) bytes = want;
        return rc;
    }
    int grow(size_t want, const char *what) { return want > bytes ? alloc(want, what) : TRACS_OK; }
    int upload(const void *host, size_t count, const char *what)
    {
        const int rc = alloc(count, what);
        if (rc) return rc;
        TRACS_HIP_CHECK(hipMemcpy(ptr, host, count, hipMemcpyHostToDevice));
        return TRACS_OK;
    }
    void *detach() { void *p = ptr; ptr = nullptr; bytes = 0; return p; }      // the block is the caller's now (device_free / pinned_free)
    template <class T> T *as() const { return static_cast<T *>(ptr); }
};
using DeviceBuffer = OwnedBuffer<false>;
using PinnedBuffer = OwnedBuffer<true>;

// the typed form: `count` elements of T.  Kernels keep taking raw pointers: pass get()
template <class T, bool kPinned = false> struct DeviceArray {
    OwnedBuffer<kPinned> buf;
    int alloc(size_t count, const char *what) { return buf.alloc(count * sizeof(T), what); }
    bool try_alloc(size_t count)
    {
        static_assert(!kPinned, "optional blocks are device memory");
        buf.release();
        if (!device_try_alloc(count * sizeof(T), &buf.ptr)) return false;
        buf.bytes = count * sizeof(T);
        return true;
    }
    T *get() const { return static_cast<T *>(buf.ptr); }
    size_t count() const { return buf.bytes / sizeof(T); }
    void release() { buf.release(); }
    T *detach() { return static_cast<T *>(buf.detach()); }
};
template <class T> using PinnedArray = DeviceArray<T, true>;

// ---- packed alignment layout -----------------------------------------------------------
// Sites are cut into groups of 128 (one uint4 = 4 x 32 sites).  For group g, plane p
// (0..3 = A,C,G,T allele planes, 4 = N plane = A&C&G&T) and sample s the 16 bytes live at
//     planes[(g * NPLANES + p) * n_pad + s]
// i.e. sample-minor, so a tile's 64..256 consecutive samples of one (group, plane) are one
// contiguous 1..4 KiB run: coalesced for the LDS stage and for the scalar row loads.
constexpr int NPLANES = 5;
constexpr int SITES_PER_GROUP = 128;
constexpr int SAMPLE_PAD = 64;       // n_pad is a multiple of one staging wave-instruction (64 samples x 16 B)
constexpr int TAIL_PAD = 512;        // zeroed uint4 behind the last plane: tiles may read (never use) up to one tile edge past n_pad
constexpr int PAD_GROUPS = 7;        // all-zero groups behind the last real one: the matrix-core kernels' stages (two groups; the
                                     // counting pass, which also reads the stored N plane in place: four, sweeps up to eight) may
                                     // overhang the alignment (zero planes contribute nothing)

static inline size_t groups_for(size_t L) { return (L + SITES_PER_GROUP - 1) / SITES_PER_GROUP; }
static inline size_t pad_samples(size_t n) { return (n + SAMPLE_PAD - 1) / SAMPLE_PAD * SAMPLE_PAD; }

}  // namespace tracs

namespace tracs { struct GeneralSparse; struct SiteLists; struct FilterIndex; }

struct tracs_alignment {
    size_t n = 0, L = 0, n_pad = 0, groups = 0;
    uint4 *planes = nullptr;     // device: general encoding, 5 planes
    uint4 *cplanes = nullptr;    // device: consensus encoding, 3 planes (derived on demand, only if valid)
    unsigned *d_flag = nullptr;  // device: "some site has a partial IUPAC code"
    bool dirty = true;           // packed since the encoding was last decided
    int enc = 0;                 // 0 general, 1 consensus
    int last_kernel = -1;        // kernel of the last dense call: 0 VALU tile kernel, 1 / 2 matrix-core kernel (consensus / one-hot)
    // Site classes (site_classes.hip), decided once per pack: a site at which every sample that is not N carries the same
    // base adds 0 to every distance and [neither is N] to every compared-sites count.  When enough sites are like that the
    // pair kernels read `vplanes` -- the alignment restricted to the DENSE sites, same encoding and layout as their usual
    // source -- and a one-operand matrix-core pass over the N plane of the other sites (`iplanes`, or the stored N plane in
    // place) completes the compared-sites counts.
    uint4 *vplanes = nullptr, *iplanes = nullptr;
    uint4 *uplane = nullptr;                  // nw_gram: "is N, or listed with w = 1 at a minority site" (one plane per group, site_classes.hip)
    bool nw_gram = false;                     // the minority sites' N x listed terms come from two one-plane matrix passes (U U^T - n n^T),
                                              // their lists hold the listed samples only (no N lists)
    bool nw_rows = false;                     // ... or, where the listed samples are few, from the rows of the site-major N matrix summed per listed
                                              // sample (site_lists.hip, minor_fixup_kernel<NSROWS>): no U plane, no second matrix pass
    size_t L_var = 0, L_inv = 0, groups_var = 0, groups_inv = 0;
    size_t L_minor = 0, L_full = 0;           // minority sites (listed in `minor`; they are part of L_un or L_full as well);
                                              // sites without any N outside vplanes: +1 to every compared-sites count
    size_t L_un = 0, L_nnl = 0;               // sites outside vplanes with an N sample (L_inv of them on the matrix cores, L_nnl
                                              // through their N lists, the rest with a single N sample: no co-occurrence)
    unsigned long long nn_visits = 0;         // list entries one pass of the N co-occurrence walk visits (sum of cN^2 over the L_nnl sites)
    unsigned long long list_entries_n = 0, list_entries_p = 0;     // 128-byte lines of the per-site N lists (primary + overflow reserve) / listed-sample entries
    unsigned long long nn_walks = 0;          // list walks of one pass of the N co-occurrence walk (sum of cN over the L_nnl sites)
    unsigned long long fix_walks = 0;         // N-list walks of one pass of the minority fix-up (listed samples of minority sites with an N sample)
    unsigned *c_counted = nullptr;            // per sample: its N sites among the sites the counting pass reads
    bool count_in_place = false;              // the counting pass reads the stored N plane of `planes` (every site) instead of iplanes:
                                              // nn = L - c_i - c_j + NN comes from it alone and the pair kernels write d only
    bool classes_cons = false;                // vplanes hold consensus planes (X, Y, V) / the five general planes
    tracs::SiteLists *lists = nullptr;        // lists of the sites with lists: minority and NNL sites (site_lists.hip)
    size_t row_hint[4] = {0, 0, 0, 0};   // tracs_alignment_hint_rows: the only rows this handle will be asked for
    int n_row_hint = 0;
    int classes_state = 0;       // 0 not decided, 1 in use, -1 not in use for this alignment
    // Arena for what is built once per pack (vplanes, iplanes, N counts, minority lists): reserved together with the planes at
    // tracs_alignment_create, because a fresh device allocation costs ~24 ms per GB on this platform (the driver clears VRAM) and
    // would otherwise land inside the first pass.  pack_alloc falls back to device_alloc when the arena is too small.
    uint8_t *arena = nullptr;
    size_t arena_bytes = 0, arena_used = 0;
    struct PackBlock { void *p; size_t bytes; };
    std::vector<PackBlock> pack_extra;       // what did not fit the arena, in use by the current pack ...
    std::vector<PackBlock> pack_spare;       // ... and released by the one before: handed out again before anything is allocated (a
                                             //   handle that is packed and called again and again -- bench.py -- would otherwise free and
                                             //   allocate gigabytes per call: ~24 ms per GB when the driver has to clear them, seconds at times)
    bool pack_oom = false;                   // a pack_alloc of the current pack failed: pack_release frees its blocks instead of parking them
    tracs::GeneralSparse *sparse = nullptr;   // general matrix-core path: per-site / per-sample lists of N and partial codes
    int sparse_state = 0;        // 0 not built, 1 built, -1 not available for this alignment (too dense / too large / no memory)
    tracs::FilterIndex *flt = nullptr;        // recombination filter: per-sample departure lists + N bitmaps (filter_lists.hip)
    bool flt_stale = true;       // packed since the filter index was built
    // cached tile schedules of the last dense regions (region x workgroup tile): the pair kernel's and the counting pass's, for
    // the two row ranges a multi-GPU rank alternates between; replaced round-robin
    struct TileCache {
        int2 *d = nullptr;
        size_t n = 0, cap = 0;
        size_t rb = (size_t)-1, re = 0, cb = 0;
        int ti = 0, tj = 0;
    } tile_cache[4];
    int tile_next = 0;
};

namespace tracs {
struct AlignmentFree { void operator()(tracs_alignment *a) const { tracs_alignment_free(a); } };
using AlignmentOwner = std::unique_ptr<tracs_alignment, AlignmentFree>;
// the HIP events of a measurement (the tracs_debug_*_timing entry points); declared before the buffers the timed kernels use
template <int N> struct OwnedEvents {
    hipEvent_t ev[N] = {};
    OwnedEvents() = default;
    OwnedEvents(const OwnedEvents &) = delete;
    OwnedEvents &operator=(const OwnedEvents &) = delete;
    ~OwnedEvents() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    int create() { for (auto &e : ev) TRACS_HIP_CHECK(hipEventCreate(&e)); return TRACS_OK; }
    hipEvent_t operator[](int k) const { return ev[k]; }
};

// what the pair kernels read: the whole alignment, or its variable sites (site classes in use)
static inline const uint4 *pair_planes(const tracs_alignment *a, bool consensus)
{
    return a->classes_state == 1 ? a->vplanes : (consensus ? a->cplanes : a->planes);
}
static inline size_t pair_L(const tracs_alignment *a) { return a->classes_state == 1 ? a->L_var : a->L; }
static inline size_t pair_groups(const tracs_alignment *a) { return a->classes_state == 1 ? a->groups_var : a->groups; }

void filter_index_free(tracs_alignment *a);        // filter_lists.hip

// site_select.hip: the kept sites of `src` packed into a new handle (tracs_alignment_select_sites); release_src_arena: `src` is about
// to be freed, its unused arena goes before the new handle is allocated
int select_sites(tracs_alignment *src, const uint64_t *keep, size_t keep_len, uint32_t max_n_samples, tracs_alignment **out,
                 uint64_t *kept, size_t *n_kept, hipStream_t stream, bool release_src_arena);

// sample_select.hip: the sample rule's counts and gather (tracs_alignment_sample_n_counts / _select_samples; release_src_arena as
// above) and the pair rule's veto pass over the cells of one dense call (tracs_pairs_min_sites; min_sites = 0: nothing is launched)
int sample_n_counts(const tracs_alignment *a, const uint64_t *keep, size_t keep_len, uint32_t *counts, hipStream_t stream);
int select_samples(tracs_alignment *src, const uint8_t *keep_sample, tracs_alignment **out, hipStream_t stream, bool release_src_arena);
int pairs_min_sites(uint32_t *dist, const uint32_t *ncomp, size_t ld, size_t n, size_t row_begin, size_t row_end, size_t col_begin,
                    int32_t dist_threshold, uint32_t min_sites, hipStream_t stream);

// msa_out.hip: the per-site census (counts device / differs host) and rows of canonical text (tracs_alignment_site_census / _unpack)
int site_census(const tracs_alignment *a, uint32_t *counts, uint64_t *differs, size_t *n_differs, hipStream_t stream);
int unpack_rows(const tracs_alignment *a, size_t first, size_t count, uint8_t *ascii, size_t stride, hipStream_t stream);

// bootstrap.hip: a replicate's column counts and its planes (tracs_bootstrap_weights / tracs_alignment_gather_sites).  bits / woff: NULL
// (weights over all L columns), or the differing-columns bitmap in 32-column words and the rank of each word's first differing column
// (weights over the differing columns only: the form tracs_distance_tree_bootstrap uses).  empty_ok: a sum of 0 leaves *out NULL;
// stage_s: NULL, or three wall times with the device drained (measurement)
int bootstrap_weights_launch(size_t L, uint64_t seed, uint64_t replicate, const unsigned *bits, const unsigned *woff, uint32_t *weights,
                             size_t weights_len, hipStream_t stream);
int gather_sites(const tracs_alignment *src, const uint32_t *weights, tracs_alignment **out, size_t *n_out, hipStream_t stream, bool empty_ok,
                 double *stage_s = nullptr);
// host only: the census bitmap `differs` (ceil(L / 64) words) as the bits / woff of bootstrap_weights_launch -> the differing columns
size_t bootstrap_column_words(const uint64_t *differs, size_t L, std::vector<unsigned> &bits, std::vector<unsigned> &woff);

// nj.hip: what the tracs_tree_write* functions write beside the tree itself (each NULL, or one value per edge), and the header of an edge
// file with those columns.  support == NULL: tracs_tree_write, byte for byte.  Else (tracs_tree_write_support) an internal node whose
// edge has a support other than 0xFFFFFFFF carries it as a decimal label, and the edge rows have a support field before ref ("NA" on
// leaf edges and where there is none).  transfer != NULL (tracs_tree_write_transfer, with support): the label is the edge's transfer
// support instead, written like a length (NaN: none), and the edge rows have a transfer field behind the support field.
// changes != NULL (tracs_tree_write_changes, without support): the edge rows have a changes field before ref; the Newick line is
// tracs_tree_write's.  filtered != NULL (tracs_tree_write_filtered, with changes): a filtered field behind the changes field.
struct TreeColumns {
    const uint32_t *support;
    const double *transfer;
    const uint32_t *changes, *filtered;
};
std::string tree_edges_header(const TreeColumns &cols);

// Four host-side checks take an edge list, each for what its caller reads out of it, and each accepts another set of lists:
//   * the loop in nj.hip's tree_write_body (tracs_tree_write*): 2n - 3 edges (n = 2: one, n < 2: none); every parent an internal node, no
//     node hung twice, a parent's rows consecutive; any number of children, in any order of the nodes -- what a Newick line can say;
//   * tree_bitsets (tracs_tree_support): n >= 4, 2n - 3 edges, no node hung twice, a parent not yet hung, an internal child already
//     given its own children -- creation order, which the bottom-up bitsets need; any number of children;
//   * transfer.hip's binary_tree_check (tracs_tree_transfer_program, tracs_transfer_init): tree_bitsets, and two children per joined
//     node, three at the top one;
//   * fitch.hip's fitch_tree_check (tracs_fitch_*): exactly the rows of tracs_nj_edges -- node n + t is the parent of rows 2t and 2t + 1,
//     the top node of the last three, children ascending within a node and older than their parent; n = 1 and n = 2 as tracs_nj_edges.
// bootstrap.hip, host only: a tree's edges checked (2n - 3 of them, creation order) and, with below != NULL, the leaves under every internal
// node v as a bitset of ceil(n / 64) words at (*below)[(v - n) * W]; kids != NULL: <- every node's number of children
int tree_bitsets(const char *who, size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges, std::vector<uint64_t> *below,
                 std::vector<uint32_t> *kids);

// transfer.hip: one replicate's program (tracs_tree_transfer_program's output, `depth` as it returned it) run against the state's main
// tree: tracs_transfer_add without the program build (tracs_distance_tree_bootstrap_transfer times the two apart)
int transfer_add_program(void *state, size_t n, const uint32_t *program, size_t depth, uint32_t *phi, hipStream_t stream);

// pair_sites.hip: the SNP sites of listed pairs (tracs_pair_sites_count / _fill) and the rows of `tracs pair-sites`
// (tracs_distance_pair_sites: names of the handle's samples, its kept-columns bitmap or NULL, the columns read)
int pair_sites_write(const tracs_alignment *a, const char *const *names, const uint64_t *kept, size_t source_len, const uint32_t *rows,
                     const uint32_t *cols, size_t n_pairs, int filter, uint64_t max_entries, const char *path, const char *const *contig_names,
                     const uint64_t *contig_lengths, size_t n_contigs, int n_threads, uint64_t *rows_written);

// fitch.hip: every site placed on a fixed tree (tracs_fitch_count / _fill) and the rows of --tree-changes / --tree-sites
// (tracs_distance_tree_changes: fitch_tables counts, the caller decides about --max-entries and writes the tree, fitch_write fills
// and formats; names, kept-columns bitmap and contigs as pair_sites_write)
struct FitchTables {
    DeviceArray<unsigned> d_edge, d_site;
    DeviceArray<uint8_t> d_min;
    DeviceArray<long long> d_off;
    std::vector<uint32_t> edge_changes;
    std::vector<long long> off;
    std::vector<uint8_t> minimum;
    uint64_t total = 0, sum_minimum = 0;
};
// the branch filter's device arrays (tracs_distance_tree_filter): the changes by edge and their verdicts
struct FitchFilter {
    const long long *d_edge_off;
    const unsigned *d_edge_site;
    const uint8_t *d_dropped;
};
int fitch_tables(const tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, FitchTables &t);
int fitch_write(const tracs_alignment *a, const char *const *names, const uint64_t *kept, size_t source_len, const uint32_t *parent,
                const uint32_t *child, size_t n_edges, const FitchTables &t, const char *changes_path, const char *sites_path, const char *ref,
                const char *const *contig_names, const uint64_t *contig_lengths, size_t n_contigs, int n_threads,
                const FitchFilter *flt = nullptr);

// fitch.hip: the tree check of tracs_fitch_* (the rows of tracs_nj_edges, nothing else) for the other files that take such a tree
int nj_tree_check(const char *who, size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges);

// tree_mask.hip: dst's planes <- src's (same n and L; tracs_alignment_clone's copy, and the restore between the iterations of
// tracs_distance_tree_iterate); dst counts as packed again.  who: the entry point an error message names
int copy_planes(const char *who, tracs_alignment *dst, const tracs_alignment *src, hipStream_t stream);
// tree_mask.hip: tracs_alignment_mask_subtrees; work (may be NULL) <- W, the (entry, leaf) cells the scatter ran over
int mask_subtrees(tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, const int64_t *edge_off,
                  const uint32_t *edge_site, const uint8_t *dropped, size_t n_entries, uint64_t *n_cells, uint64_t *work, hipStream_t stream);

// device memory that lives until the alignment is packed again (site_classes_free releases all of it at once)
bool pack_alloc(tracs_alignment *a, size_t bytes, void **out);      // false: no memory (never an error: the callers fall back)
void pack_release(tracs_alignment *a);

// Grow-only per-device scratch buffers, shared by every entry point.  Every slot of every file is declared here, once: a new buffer
// takes a new name in its owner's group (the values are the library's own; nothing outside it sees them).
enum WsSlot : int {
    // transcluster.hip: the distinct (N, delta) keys of one call, their results and the optional (gap, M) / grid tables
    WS_TC_SLOTS, WS_TC_ESLOT, WS_TC_SLOT_ID, WS_TC_NKEYS, WS_TC_KEY_ELEM, WS_TC_KEY_P0, WS_TC_KEY_EK, WS_TC_LONG_IDS, WS_TC_KEY_STATE,
    WS_TC_TAB, WS_TC_TAB_LNS, WS_TC_TAB_POIS, WS_TC_GRID_BITS, WS_TC_GRID_TABLES, WS_TC_TAB_LNS_N, WS_TC_REST_IDS,
    // transcluster.hip: the key split between ranks (tracs_trans_keys_*)
    WS_KS_RANK, WS_KS_CHUNK, WS_KS_INFO,
    // cluster.hip: union-find parents, root flags, roots, the component count
    WS_CC_PARENT, WS_CC_FLAG, WS_CC_ROOT, WS_CC_TOTAL,
    // dmultinomial.hip: the posterior table
    WS_DM_TABLE,
    // dirichlet.hip: count rows, per-block partial sums, kept rows, the fit's state, block counts (consecutive: used in this order)
    WS_DIR_ROWS, WS_DIR_PARTIAL, WS_DIR_NKEPT, WS_DIR_STATE, WS_DIR_BLOCKS,
    // site_lists.hip: the site-major N matrix of the rows fix-up
    WS_SL_NROWS,
    // pairsnp.hip: live tiles of a thresholded dense call
    WS_PS_LIVE, WS_PS_LIVE_TILES, WS_PS_N_LIVE,
    // site_classes.hip: per-group masks, offsets and counts of the class decision, and the dense / counted site lists
    WS_SC_MASKS, WS_SC_OFFS, WS_SC_CNTS, WS_SC_GCNT, WS_SC_OFF64, WS_SC_TOTALS, WS_SC_FLAGS, WS_SC_LISTS,
    // site_lists.hip: per-sample counts, per-group entry counts, the entries and (optional) their second sorting buffer
    WS_SL_CNT, WS_SL_ECNT, WS_SL_ENTRIES, WS_SL_ENTRIES_TMP,
    // pair_sites.hip: tile sums of the offsets scan, the bad-pair flag
    WS_PSITES_SUMS, WS_PSITES_BAD,
    // filter_lists.hip: the index build's per-chunk counts and the departure scratch of a filter pass
    WS_FLT_CNT, WS_FLT_REL, WS_FLT_TOT, WS_FLT_STATS, WS_FLT_IDX, WS_FLT_SCRATCH,
    // filter.hip: SNP positions of the listed pairs and their offsets scan
    WS_FSCAN_POS, WS_FSCAN_FOUND, WS_FSCAN_OFF, WS_FSCAN_SUMS,
    // forest.hip: the two working edge lists, the new forest's sources and values, emit's sort keys and indices
    WS_MSF_W0, WS_MSF_W1, WS_MSF_FSRC, WS_MSF_FTMP, WS_MSF_SORT_KEYS, WS_MSF_SORT_IDX, WS_MSF_SORT_TMP,
    // msa_out.hip: the differs bitmap of the site census
    WS_MSA_DIFFERS,
    // ancestors.hip: the radix sort's temporary storage
    WS_ANC_SORT_TMP,
    // bootstrap.hip: the scanned column counts of a replicate and the first source column of every output group
    WS_BS_OFFSETS, WS_BS_STARTS,
    // fitch.hip: a slab's node sets [node][word], the edge list's child column, tile sums of the offsets scan; the [chunk][edge] matrix of
    // tracs_fitch_edge_sites and its per-edge cursor
    WS_FITCH_NODES, WS_FITCH_TREE, WS_FITCH_SUMS, WS_FITCH_MATRIX, WS_FITCH_CURSOR,
    // tree_mask.hip: the leaf order and the edges' intervals in it, per entry its weight and its interval's start, the scanned weights
    // and their tile sums, the count of newly masked cells
    WS_MASK_TREE, WS_MASK_WEIGHT, WS_MASK_LO, WS_MASK_OFF, WS_MASK_SUMS, WS_MASK_CELLS,
    WS_SLOT_COUNT
};

// Entry points that use scratch buffers, or the cached state of a tracs_alignment, hold a DeviceCall for their whole body:
//   * calls on one device are serialised (ctypes releases the GIL, so two Python threads can be inside the library);
//   * scratch is only stream-ordered, so when a call arrives on a different stream than the previous call on that device
//     the device is synchronised first.  Re-entrant on the owning thread (tracs_pairsnp calls the dense entry points).
int workspace_bytes(WsSlot slot, size_t bytes, void **out);        // (capi.hip; callers use the typed forms below)
// *out <- the slot's buffer, at least `count` elements of T
template <class T>
static int workspace_get(WsSlot slot, size_t count, T **out)
{
    return workspace_bytes(slot, count * sizeof(T), reinterpret_cast<void **>(out));
}
// an optional buffer: not getting it is not an error.  false leaves *out NULL, the error slot and HIP's last error clear
template <class T>
static bool workspace_try(WsSlot slot, size_t count, T **out)
{
    if (workspace_get(slot, count, out) == TRACS_OK) return true;
    (void)hipGetLastError();
    set_error("");
    *out = nullptr;
    return false;
}
void workspace_release_all();
struct DeviceCall {
    explicit DeviceCall(hipStream_t stream);
    ~DeviceCall();
    DeviceCall(const DeviceCall &) = delete;
    DeviceCall &operator=(const DeviceCall &) = delete;
    int dev;
};
}  // namespace tracs
