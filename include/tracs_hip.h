/*
 * tracs_hip.h -- C ABI of libtracs_hip.so, the MI355X (gfx950) implementation of the TRACS
 * all-pairs distance path.  Plain pointers and sizes only; no C++ or torch types.
 *
 * Two layers:
 *   (1) HOST entry points -- exactly what the reference's pybind11 module binds
 *       (/root/reference/src/python_bindings.cpp:12-25).  Host pointers in, host pointers out.
 *   (2) DEVICE entry points -- the same kernels with device pointers and a hipStream_t
 *       (passed as void*), for callers that keep the alignment resident in HBM (bench.py,
 *       the multi-GPU driver, `tracs distance`).  Asynchronous on the given stream.
 *
 * Threading: entry points that run kernels are serialised per device inside the library (scratch buffers and the cached
 * state of a tracs_alignment are shared), and scratch is stream-ordered: a call that arrives on a different stream than
 * the previous call on that device synchronises the device first.  Use one stream per device for overlap-free pipelines.
 *
 * Every function returns 0 on success or a negative TRACS_E_* code; tracs_last_error()
 * returns the message for the calling thread (the Python layer raises RuntimeError with it,
 * reproducing the reference's messages: src/pairsnp.hpp:86,90,96-97,342).
 */
#ifndef TRACS_HIP_H
#define TRACS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRACS_OK            0
#define TRACS_E_ARG        -1   /* bad argument (e.g. "Invalid number of fasta files!") */
#define TRACS_E_FASTA      -2   /* "Error reading FASTA!"                        (pairsnp.hpp:86,90) */
#define TRACS_E_RAGGED     -4   /* "Error reading FASTA, variable sequence lengths!" (pairsnp.hpp:96-97) */
#define TRACS_E_OPEN       -5   /* file cannot be opened (the reference does not diagnose this) */
#define TRACS_E_HIP        -6   /* HIP runtime error / no device */
#define TRACS_E_NOMEM      -7
#define TRACS_E_INTERRUPTED -8  /* "Interrupted by user!" (SIGINT during tracs_pairsnp; pairsnp.hpp:434-441 exits instead) */

const char *tracs_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int tracs_abi_version(void);
/* Number of visible HIP devices (<=0: none).  Does not throw. */
int tracs_device_count(void);

/* ===================================================================================== */
/* (1) HOST ENTRY POINTS -- the pybind11 surface                                          */
/* ===================================================================================== */

/* pairsnp(fasta, n_threads, dist, filter)
 *   replaces: src/python_bindings.cpp:12-13 -> src/pairsnp.hpp:320-457.
 *   fasta: 1 path (all i<j) or 2 paths (file0 x file1 only, pairsnp.hpp:352-360); plain or gzip.
 *   n_threads: accepted for signature parity; the pair loop runs on the GPU.
 *   dist: emit pairs with d <= dist (signed int compare, pairsnp.hpp:405).
 *   filter: recombination filter (pairsnp.hpp:251-318; pinned to its definition); 0 => filt_distances are `len` zeros
 *           (pairsnp.hpp:452 with combine_vectors :31).
 * The result is an opaque handle read through the accessors below; rows/cols/... are
 * row-major (i, then j) like the reference (pairsnp.hpp:451-455).                         */
typedef struct tracs_pairsnp_result tracs_pairsnp_result;
int tracs_pairsnp(const char *const *fasta, int n_fasta, int n_threads, int dist, int filter,
                  tracs_pairsnp_result **out);
size_t tracs_pairsnp_len(const tracs_pairsnp_result *r);          /* number of emitted pairs */
size_t tracs_pairsnp_nseq(const tracs_pairsnp_result *r);         /* records loaded, both files */
size_t tracs_pairsnp_seqlen(const tracs_pairsnp_result *r);       /* alignment length L */
const uint64_t *tracs_pairsnp_rows(const tracs_pairsnp_result *r);
const uint64_t *tracs_pairsnp_cols(const tracs_pairsnp_result *r);
const uint64_t *tracs_pairsnp_distances(const tracs_pairsnp_result *r);
const uint64_t *tracs_pairsnp_filt_distances(const tracs_pairsnp_result *r);
const uint64_t *tracs_pairsnp_ncompared(const tracs_pairsnp_result *r);
const char *tracs_pairsnp_name(const tracs_pairsnp_result *r, size_t i);
void tracs_pairsnp_free(tracs_pairsnp_result *r);

/* Per-sample k nearest neighbours (not in the reference).  The candidates of sample s are ranked by the key
 * (d, j): SNP distance first, then the candidate's sample index, a total order.  One file: every j != s (the same pair can come
 * back under each of its samples).  Two files: only the samples of file 0 get lists, their candidates are the samples of file 1.
 * Only pairs with d <= dist are eligible; each sample keeps min(k, eligible) neighbours, 1 <= k <= 1024 (else TRACS_E_ARG).
 * The result is read through the tracs_pairsnp_* accessors: rows = s ascending, then the key ascending; cols = j, d, nn exact;
 * filter != 0: the filtered distances of the emitted pairs (selection always uses the raw d), else zeros.  n_threads is accepted
 * for signature parity with tracs_pairsnp and unused: every stage runs on the GPU.                                           */
int tracs_nearest(const char *const *fasta, int n_fasta, int n_threads, int k, int dist, int filter,
                  tracs_pairsnp_result **out);

/* tracs_pairsnp / tracs_nearest under a site rule (tracs_alignment_select_sites: keep over the columns of the files, NULL = all;
 * max_n_samples counted over every loaded sample, both files of a two-file run; UINT32_MAX = no rule): the result is that of the
 * files with the dropped columns deleted, tracs_pairsnp_seqlen the number of kept columns.  Without any rule: the plain entry
 * points, call for call.                                                                                                     */
int tracs_pairsnp_sites(const char *const *fasta, int n_fasta, int n_threads, int dist, int filter, const uint64_t *keep,
                        size_t keep_len, uint32_t max_n_samples, tracs_pairsnp_result **out);
int tracs_nearest_sites(const char *const *fasta, int n_fasta, int n_threads, int k, int dist, int filter, const uint64_t *keep,
                        size_t keep_len, uint32_t max_n_samples, tracs_pairsnp_result **out);

/* trans_dist(snpdiff, datediff, lamb, beta, threshold_Ek) -> (p0_log[n], eK[n])
 *   replaces: src/python_bindings.cpp:19-21 -> src/transcluster.hpp:240-287.               */
int tracs_trans_dist(const int32_t *snpdiff, const double *datediff, size_t n, double lamb, double beta,
                     double threshold_Ek, double *p0_log, double *eK);

/* lprob_k_given_N(N, k, delta, lamb, beta, lgamma) -> (lprob, lhs)
 *   replaces: src/python_bindings.cpp:15-17 -> src/transcluster.hpp:90-129.
 *   lgamma[i] = ln Gamma(i), length > N+k+1 (caller supplied, as in tests/test_llk.py:26).
 *   Batched: n independent (N,k,delta) triples share lamb, beta and the table.             */
int tracs_lprob_k_given_N(const uint64_t *N, const uint64_t *k, const double *delta, size_t n, double lamb,
                          double beta, const double *lgamma, size_t lgamma_len, double *lprob, double *lhs);

/* calculate_posteriors(counts[L,K], alphas[K], keep, threshold) -> posterior[L,K]
 *   replaces: src/python_bindings.cpp:23-25 -> src/dmultinomial.hpp:8-86.  K <= 8.          */
int tracs_calculate_posteriors(const double *counts, size_t L, size_t K, const double *alphas, int keep,
                               double threshold, double *posterior);

/* find_dirichlet_priors(counts[L,K], max_iter, tol, method, error_filt_threshold) -> alphas[K] (descending)
 *   replaces: tracs/dirichlet_multinomial.py:9-73 (the fit whose output calculate_posteriors consumes,
 *   tracs/align.py:536-538).  method 0 = Minka fixed point (the reference's default branch), 1 = leave-one-out;
 *   error_filt_threshold < 0 = None.  Fewer than 6 polymorphic sites -> (0,..,0,1) like the reference.        */
int tracs_find_dirichlet_priors(const double *counts, size_t L, size_t K, int max_iter, double tol, int method,
                                double error_filt_threshold, double *alphas_out, int *iters_out);

/* Threshold single-linkage clustering = connected components of the edge list, labelled as
 * scipy.sparse.csgraph.connected_components(directed=False) labels them
 *   replaces: tracs/cluster.py:126-129.  edges (I[e], J[e]) over nodes 0..n-1.             */
int tracs_connected_components(const int32_t *I, const int32_t *J, size_t n_edges, size_t n_nodes,
                               int32_t *labels, int32_t *n_components);

/* ===================================================================================== */
/* (2) DEVICE ENTRY POINTS                                                                */
/* ===================================================================================== */

/* A packed alignment resident in HBM: five bit planes (A,C,G,T and N = A&C&G&T) per sample,
 * 128-site groups, sample-minor: uint4[group][plane][n_pad] (DESIGN.md "Data layout").     */
typedef struct tracs_alignment tracs_alignment;
int tracs_alignment_create(size_t n, size_t L, tracs_alignment **out);
void tracs_alignment_free(tracs_alignment *a);
size_t tracs_alignment_n(const tracs_alignment *a);
size_t tracs_alignment_len(const tracs_alignment *a);
size_t tracs_alignment_bytes(const tracs_alignment *a);   /* HBM bytes of the packed planes */
void *tracs_alignment_planes(const tracs_alignment *a);   /* device pointer of the packed planes (tracs_alignment_bytes long) */
/* The planes were written through that pointer from outside the library (e.g. an RCCL broadcast from the rank that packed):
 * forget every cached derived form (consensus planes, sparse lists, tile schedule stay valid per geometry).          */
int tracs_alignment_touch(tracs_alignment *a);
/* Multi-GPU ranks (every rank holds the whole alignment and computes its row panels): this handle will only be
 * asked for rows inside the given [begin, end) ranges (up to 2; n_ranges = 0 lifts the promise).  What is built once per pack
 * PER ROW -- the per-sample lists of the site classes -- is then built for those rows only (1 / ranks of that work); a dense
 * call for other rows fails with TRACS_E_ARG rather than returning results from lists that were never built.                */
int tracs_alignment_hint_rows(tracs_alignment *a, const size_t *ranges, int n_ranges);
/* Pack `count` samples of ASCII (IUPAC, any case; load_seqs pairsnp.hpp:107-199) into samples
 * [first, first+count).  `ascii` is count*L bytes, row-major; host or device pointer
 * (ascii_on_device).  The pack itself is a HIP kernel either way.                           */
int tracs_alignment_pack(tracs_alignment *a, const uint8_t *ascii, size_t first, size_t count,
                         int ascii_on_device, void *stream);
/* Read FASTA/FASTQ(.gz) with kseq semantics (src/kseq.h:170-208) and pack it.  names_out
 * receives a malloc'ed block of NUL-separated names (free with tracs_free).                 */
int tracs_alignment_from_fasta(const char *const *fasta, int n_fasta, tracs_alignment **out,
                               char **names_out, size_t *names_bytes, size_t *n_first_file);
void tracs_free(void *p);

/* Site rules (not in the reference).  A run with a site rule is, by definition, the run on the alignment with the
 * dropped columns deleted from every record: the kept columns are packed into a new handle that is byte for byte what packing the
 * column-deleted text gives, and every other entry point runs on that handle unchanged.
 *   tracs_alignment_site_n_counts  per site, the samples that are N there (bit set in the stored N plane: 'N', '-' and every byte
 *                                  that is not an IUPAC letter; partial codes are not N) -> counts, device uint32[L]
 *   tracs_alignment_select_sites   keep: host bitmap, bit s of keep[s / 64] = site s may stay; NULL = all.  keep_len must equal the
 *                                  handle's length.  max_n_samples: a site stays only if at most that many samples are N there;
 *                                  UINT32_MAX = no rule.  *out: a NEW handle over the kept columns (src is left as it was and stays
 *                                  usable).  kept (host, ceil(L / 64) words, may be NULL) receives the final bitmap, *n_kept its
 *                                  population.  A rule that leaves no site is refused (TRACS_E_ARG, "no site left after the site
 *                                  rules").  Synchronises the stream.                                                        */
int tracs_alignment_site_n_counts(const tracs_alignment *a, uint32_t *counts, void *stream);
int tracs_alignment_select_sites(const tracs_alignment *src, const uint64_t *keep, size_t keep_len, uint32_t max_n_samples,
                                 tracs_alignment **out, uint64_t *kept, size_t *n_kept, void *stream);

/* Sample rule and pair rule (not in the reference).  A run with the sample rule is, by definition, the run on the FASTA
 * file(s) with the dropped records deleted: the kept samples are gathered into a new handle that is byte for byte what packing the
 * record-deleted text gives (pad samples, tail bits, pad groups and slack zero; n_pad may shrink), and every other entry point runs
 * on that handle unchanged.  The pair rule is one pass over a dense panel before anything reads it.
 *   tracs_alignment_sample_n_counts  per sample, the sites at which it is N (the stored N plane, as tracs_alignment_site_n_counts)
 *                                    among the columns `keep` leaves (host bitmap as tracs_alignment_select_sites takes it, keep_len
 *                                    = the handle's length; NULL: every column) -> counts, device uint32[n].  Exact (integer sums).
 *                                    With a bitmap the call synchronises the stream.
 *   tracs_alignment_select_samples   keep_sample: host uint8[n], non-zero = the sample stays.  *out: a NEW handle over the kept
 *                                    samples in their order (src is left as it was and stays usable).  A mask that keeps nothing is
 *                                    refused (TRACS_E_ARG, "no sample left after the sample rule").  Synchronises the stream.
 *   tracs_pairs_min_sites            the cells of one dense call -- rows [row_begin, row_end), columns [max(col_begin, i + 1), n) of
 *                                    dist / ncomp (device uint32, indexed by ABSOLUTE row, leading dimension ld >= n): a cell whose
 *                                    distance, read unsigned, is <= dist_threshold and whose ncomp is < min_sites gets the distance
 *                                    0xFFFFFFFF, which tracs_coo_count / _fill, tracs_knn_update, tracs_hist_update and the
 *                                    transcluster entry points read as "beyond the threshold".  Every other cell, ncomp and every
 *                                    byte outside the cell set stay as they were.  min_sites = 0: nothing is launched.             */
int tracs_alignment_sample_n_counts(const tracs_alignment *a, const uint64_t *keep, size_t keep_len, uint32_t *counts, void *stream);
int tracs_alignment_select_samples(const tracs_alignment *src, const uint8_t *keep_sample, tracs_alignment **out, void *stream);
int tracs_pairs_min_sites(uint32_t *dist, const uint32_t *ncomp, size_t ld, size_t n, size_t row_begin, size_t row_end, size_t col_begin,
                          int32_t dist_threshold, uint32_t min_sites, void *stream);

/* The alignment a run compared, back as text, and what is in its columns (not in the reference).  Masks are the
 * pack's: bit 0 = A, 1 = C, 2 = G, 3 = T.  The canonical letter of a mask m is "XACMGRSVTWYHKDBN"[m] (15 -> 'N'): lower case, '-' and
 * non-letters come out as their upper-case letter or 'N', and packing the canonical text of a handle gives the handle's bytes back.
 *   tracs_alignment_site_census  per site, over the handle's n samples (pad samples never count): counts (device uint32, category-
 *                                major counts[c * L + s], c = A, C, G, T, N, other: the samples whose mask is exactly that letter,
 *                                all four bits, or a partial code; the six sum to n; may be NULL) and whether the site DIFFERS:
 *                                two samples have disjoint masks there (m_i & m_j == 0) -- exactly the sites that add 1 to some
 *                                d(i, j).  differs (host bitmap, ceil(L / 64) words, bit s of differs[s / 64]; may be NULL),
 *                                *n_differs its population (may be NULL).  Synchronises the stream when either is asked for.
 *   tracs_alignment_unpack       samples [first, first + count) -> canonical text, device uint8, row k at ascii + k * stride.  Writes
 *                                the L bytes of each row and nothing else (no byte at or beyond column L, no other row).  Refused
 *                                with TRACS_E_ARG, nothing launched: first + count > n, stride < L, a NULL pointer.               */
int tracs_alignment_site_census(const tracs_alignment *a, uint32_t *counts, uint64_t *differs, size_t *n_differs, void *stream);
int tracs_alignment_unpack(const tracs_alignment *a, size_t first, size_t count, uint8_t *ascii, size_t stride, void *stream);

/* The rules of the FASTA entry points in one place.  Applied in this order:
 *   1. keep / keep_len       the file rules' bitmap over the columns read (NULL: every column); L' = the columns it leaves
 *   2. max_sample_n_share G  a record is left out when more than floor(G L') of those columns are N in it; with two files the rule
 *                            applies to both and the first file's count shrinks; a file left without a record is refused
 *                            (TRACS_E_ARG, "no sample left after the sample rule").  G = 1 drops nothing.  < 0: no rule
 *   3. max_n_share F         a column is dropped when more than floor(F n') of the n' SURVIVING samples are N there (computed in the
 *                            library as floor(F * (double)n'), once n' is known).  < 0: no rule.  max_n_samples: the same rule
 *                            with the threshold given (UINT32_MAX: no rule); giving both is refused
 *   4. min_sites M           a pair is eligible only if its compared-sites count over the kept columns is >= M (tracs_pairs_min_sites
 *                            on every dense panel).  0: no rule
 * A struct without any rule (or NULL) is call for call the plain entry point.                                                    */
typedef struct tracs_rules {
    const uint64_t *keep;
    size_t keep_len;
    double max_n_share;
    double max_sample_n_share;
    uint32_t min_sites;
    uint32_t max_n_samples;
} tracs_rules;
int tracs_pairsnp_rules(const char *const *fasta, int n_fasta, int n_threads, int dist, int filter, const tracs_rules *rules,
                        tracs_pairsnp_result **out);
int tracs_nearest_rules(const char *const *fasta, int n_fasta, int n_threads, int k, int dist, int filter, const tracs_rules *rules,
                        tracs_pairsnp_result **out);
/* What the sample rule saw, on a result: the records read in input order (both files), each one's N sites among the L' file-kept
 * columns (tracs_pairsnp_rule_sites), and whether it stayed.  tracs_pairsnp_nseq / _name are the SURVIVING samples, the ones rows and
 * cols index.  Without a sample rule: the loaded samples, all kept, counts 0.                                                     */
size_t tracs_pairsnp_source_nseq(const tracs_pairsnp_result *r);
const char *tracs_pairsnp_source_name(const tracs_pairsnp_result *r, size_t i);
uint32_t tracs_pairsnp_source_n_count(const tracs_pairsnp_result *r, size_t i);
int tracs_pairsnp_source_kept(const tracs_pairsnp_result *r, size_t i);
size_t tracs_pairsnp_rule_sites(const tracs_pairsnp_result *r);

/* Dense pair block: for rows i in [row_begin,row_end) and columns j in [max(col_begin,i+1), n)
 *   dist[i*ld + j]  = d(i,j)  = L - popcount(match)           (pairsnp.hpp:398-403)
 *   ncomp[i*ld + j] = nn(i,j) = L - popcount(N_i | N_j)       (pairsnp.hpp:417-420)
 * Other cells are not written.  dist/ncomp are device uint32 matrices with leading dimension
 * ld >= n; ncomp may be NULL (then only d is written).                                           */
int tracs_pairsnp_dense(const tracs_alignment *a, size_t row_begin, size_t row_end, size_t col_begin,
                        uint32_t *dist, uint32_t *ncomp, size_t ld, void *stream);

/* Two streams.  The distances of a dense call are final before its compared-sites counts are (site classes: the counting pass and
 * the N co-occurrence walk only touch ncomp), and transcluster reads distances only.
 *   tracs_pairsnp_notify_distances(event)  the NEXT dense call on this thread's device records `event` (a hipEvent_t) on its
 *                                          stream once `dist` is final; a second stream that waits on it can run
 *                                          tracs_trans_dist_dense* beside the rest of the call (bench.py: memory-bound list walk and
 *                                          f64-bound key evaluation overlap);
 *   tracs_set_stream_policy(1)             the caller orders its streams itself (events).  Default 0: a call that arrives on another
 *                                          stream than the previous call on the device synchronises the device first, because the
 *                                          library's scratch buffers are only stream-ordered.  With policy 1 calls that share
 *                                          scratch (two transcluster calls; two first-calls on freshly packed handles; two
 *                                          posterior-codes calls with different parameters: their per-total table; two dense calls
 *                                          on alignments with minority lists: the fix-up's scratch rows) must be ordered by the
 *                                          caller; a dense call on a decided handle and a transcluster call share none. */
void tracs_pairsnp_notify_distances(void *event);
void tracs_set_stream_policy(int caller_orders_streams);

/* Thresholded form: identical (d and nn) for every pair with d <= dist_threshold.  A pair beyond the threshold (never
 * emitted, src/pairsnp.hpp:405) may come back with bit 31 of its distance set (0xFFFFFFFF, or a partial count | 2^31), or
 * (general alignments, and alignments cut into site classes) with a value > threshold that is not its distance, and an unspecified ncomp,
 * because workgroups stop reading the alignment once every pair of their tile is past the threshold: a pair is within the
 * threshold iff its cell, read as an UNSIGNED 32-bit value, is <= dist_threshold (what tracs_coo_count/fill test).
 * Long alignments take two passes (a 1/8 prefix over all tiles, then the rest over the surviving tiles only); this call
 * synchronises the stream once between them.                                                                          */
int tracs_pairsnp_dense_thr(const tracs_alignment *a, size_t row_begin, size_t row_end, size_t col_begin,
                            uint32_t *dist, uint32_t *ncomp, size_t ld, int32_t dist_threshold, void *stream);

/* Thresholded COO extraction from a dense block, row-major, same cell set as above.
 * Phase 1 (counts==per-row counts, device int64[row_end-row_begin+1] exclusive offsets on return),
 * phase 2 fills rows/cols/d/nn (device uint32) at those offsets.                            */
int tracs_coo_count(const uint32_t *dist, size_t ld, size_t n, size_t row_begin, size_t row_end,
                    size_t col_begin, int32_t dist_threshold, int64_t *offsets, void *stream);
int tracs_coo_fill(const uint32_t *dist, const uint32_t *ncomp, size_t ld, size_t n, size_t row_begin,
                   size_t row_end, size_t col_begin, int32_t dist_threshold, const int64_t *offsets,
                   uint32_t *rows, uint32_t *cols, uint32_t *d, uint32_t *nn, void *stream);
/* ... and two float64 panels of the same geometry (P(direct), E(K) as tracs_trans_dist_dense writes them) into the same positions */
int tracs_coo_fill_f64(const uint32_t *dist, size_t ld, size_t n, size_t row_begin, size_t row_end, size_t col_begin,
                       int32_t dist_threshold, const int64_t *offsets, const double *a, const double *b, double *out_a,
                       double *out_b, void *stream);

/* Threshold edges of a float64 panel (E(K) or P(direct) as written by tracs_trans_dist_dense; what `tracs cluster -D
 * expectedK|direct -c T` keeps, tracs/cluster.py:110-112): cells (i, j) of the same cell set whose SNP distance was emitted
 * (dist <= dist_threshold) and whose value is <= threshold, row-major.  Same two phases as tracs_coo_count/fill; vals (the
 * kept values) may be NULL.  This is the per-rank edge list the multi-GPU clustering path gathers.       */
int tracs_edges_count_f64(const double *val, const uint32_t *dist, size_t ld, size_t n, size_t row_begin, size_t row_end,
                          size_t col_begin, int32_t dist_threshold, double threshold, int64_t *offsets, void *stream);
int tracs_edges_fill_f64(const double *val, const uint32_t *dist, size_t ld, size_t n, size_t row_begin, size_t row_end,
                         size_t col_begin, int32_t dist_threshold, double threshold, const int64_t *offsets, uint32_t *rows,
                         uint32_t *cols, double *vals, void *stream);

/* k-nearest-neighbour selection over dense panels (csrc/nearest.hip; what tracs_nearest runs).  The state is a device buffer of
 * tracs_knn_state_bytes(n_lists, k) bytes holding one running list per sample of [0, n_lists): the k smallest keys (d, j) offered
 * so far with their compared-site counts.
 *   tracs_knn_init    every list empty
 *   tracs_knn_update  merge the panel rows [row_begin, row_end) of dist / ncomp (tracs_pairsnp_dense[_thr]'s cells: columns
 *                     j >= max(col_begin, i + 1), indexed by ABSOLUTE row, leading dimension ld) into the lists: row i offers
 *                     (d(i, j), j) to list i; with symmetric != 0 (one-file mode) column c also offers (d(i, c), i) to list c.  A
 *                     cell is eligible iff it is, read as unsigned, <= dist_threshold.  The state must hold lists for row_end
 *                     samples (n with symmetric).  Every cell is offered at most once over the updates of one state: panels do not
 *                     overlap.  Two stream-ordered launches; nn is read for the kept cells while the panel is resident.
 *   tracs_knn_emit    lists [list_begin, list_end) -> offsets (device int64[list_end - list_begin + 1], exclusive: list s's
 *                     neighbours are entries offsets[s - list_begin] ..) and, unless all four are NULL, rows / cols / d / nn
 *                     (device uint32, room for (list_end - list_begin) * k entries) in list order, each list by key.          */
size_t tracs_knn_state_bytes(size_t n_lists, int k);
int tracs_knn_init(void *state, size_t n_lists, int k, void *stream);
int tracs_knn_update(const uint32_t *dist, const uint32_t *ncomp, size_t ld, size_t n, size_t row_begin, size_t row_end,
                     size_t col_begin, int32_t dist_threshold, int k, int symmetric, void *state, void *stream);
int tracs_knn_emit(void *state, size_t list_begin, size_t list_end, int k, int64_t *offsets, uint32_t *rows, uint32_t *cols,
                   uint32_t *d, uint32_t *nn, void *stream);

/* Minimum spanning forest of the offered pairs (csrc/forest.hip; what tracs_distance_forest runs).  Pairs are ordered
 * by (weight, i, j), i < j their sample indices: uint32 weights as numbers; f64 weights as numbers with -0.0 == +0.0 and every NaN
 * above +inf.  A total order, so the forest is unique and independent of how the pairs are split into updates.  The state is a device
 * buffer of tracs_msf_state_bytes(n) bytes for the vertices [0, n): the running forest (< n edges, each with the values its row is
 * written with: d, nn, filtered d, P, E(K)) and per-vertex scratch.
 *   tracs_msf_init        the empty forest
 *   tracs_msf_update_coo  F <- MSF(F u batch): m pairs (rows[t], cols[t]) (device uint32, either order, an endpoint >= n or a loop
 *                         is skipped) with weight[t] (device; weight_kind 0: uint32, 1: double); e_mask != NULL: only pairs with
 *                         e_max >= e_mask[t] are eligible (a NaN fails); d / nn / filt / p / e (device, any may be NULL: stored as
 *                         0) are the values kept with a pair.  Every pair is offered at most once over the updates of one state.
 *                         n_taken (host, optional): the batch's eligible pairs.  Boruvka rounds on the device, one word read per
 *                         round; synchronises the stream.
 *   tracs_msf_emit        *n_edges <- the forest's size; unless NULL, rows < cols, d, nn, filt (device uint32) and p, e (device
 *                         double), room for n - 1 entries, receive the forest in (i, j) order.  Synchronises the stream.        */
size_t tracs_msf_state_bytes(size_t n);
int tracs_msf_init(void *state, size_t n, void *stream);
int tracs_msf_update_coo(void *state, size_t n, size_t m, const uint32_t *rows, const uint32_t *cols, const void *weight, int weight_kind,
                         const double *e_mask, double e_max, const uint32_t *d, const uint32_t *nn, const uint32_t *filt,
                         const double *p, const double *e, uint64_t *n_taken, void *stream);
int tracs_msf_emit(void *state, size_t n, size_t *n_edges, uint32_t *rows, uint32_t *cols, uint32_t *d, uint32_t *nn, uint32_t *filt,
                   double *p, double *e, void *stream);

/* Each vertex's most likely earlier source among the offered pairs (csrc/ancestors.hip; what tracs_distance_ancestors runs; DESIGN.md
 * 3.16).  Vertex s has the day days[s]; vertex a is a candidate source of s when {a, s} is an offered, eligible pair and
 * days[a] < days[s], strictly.  The chosen source is the smallest candidate under (value key, days[s] - days[a], a): a total order, so
 * the result is independent of how the pairs are split into updates.  A vertex without a candidate is a root.  The state is a device
 * buffer of tracs_anc_state_bytes(n) bytes for the vertices [0, n): the days, per vertex the running best keys and the winning pair
 * with the values its row is written with (d, nn, filtered d, P, E(K)), and scratch for emit.
 *   tracs_anc_init        no pair offered yet; days_device: device int32[n] (days since 1970-01-01, negative ones too), copied
 *   tracs_anc_update_coo  offer m pairs (rows[t], cols[t]) (device uint32, either order; an endpoint >= n, a loop or a pair with equal
 *                         days is skipped) with value[t] (device; value_kind 0: uint32 ascending; 1: double ascending, -0.0 == +0.0,
 *                         every NaN above +inf; 2: double DESCENDING, -0.0 == +0.0, every NaN after -inf); e_mask != NULL: only pairs
 *                         with e_max >= e_mask[t] are eligible (a NaN fails); d / nn / filt / p / e (device, any may be NULL: stored
 *                         as 0) are the values kept with a pair.  Every pair is offered at most once over the updates of one state.
 *                         n_taken (host, optional): the candidates offered -- the batch's eligible pairs with unequal days; reading
 *                         it synchronises the stream.  Five stream-ordered launches, one atomic target per pair.
 *   tracs_anc_emit        *n_links <- the number of vertices with a source; unless NULL, rows < cols, d, nn, filt (device uint32) and
 *                         p, e (device double), room for n - 1 entries, receive the links in (i, j) order; unless NULL, parent, root
 *                         and generation (device uint32[n]) receive per vertex its source (0xFFFFFFFF for a root), the vertex reached
 *                         by following sources, and the number of links to it (pointer doubling, ceil(log2 n) rounds).  Synchronises
 *                         the stream.                                                                                            */
size_t tracs_anc_state_bytes(size_t n);
int tracs_anc_init(void *state, size_t n, const int32_t *days_device, void *stream);
int tracs_anc_update_coo(void *state, size_t n, size_t m, const uint32_t *rows, const uint32_t *cols, const void *value, int value_kind,
                         const double *e_mask, double e_max, const uint32_t *d, const uint32_t *nn, const uint32_t *filt,
                         const double *p, const double *e, uint64_t *n_taken, void *stream);
int tracs_anc_emit(void *state, size_t n, size_t *n_links, uint32_t *rows, uint32_t *cols, uint32_t *d, uint32_t *nn, uint32_t *filt,
                   double *p, double *e, uint32_t *parent, uint32_t *root, uint32_t *generation, void *stream);

/* Neighbour joining on the dense distance matrix (csrc/nj.hip; what tracs_distance_tree runs).  Canonical neighbour
 * joining (Saitou & Nei, Q as Studier & Keppler) in IEEE float64 with every operation and its order fixed and no fused multiply-add, so
 * that a restatement on the host gives the same bits.  Leaves are the nodes [0, n); join number t makes the node n + t.  With r active
 * nodes: Q_ab = (r - 2) D_ab - (R_a + R_b); the join is the smallest (Q, lower id, higher id); D_uk = ((D_ak + D_bk) - D_ab) / 2;
 * R_k <- (R_k - (D_ak + D_bk)) + D_uk; R_u = ((R_a + R_b) - r D_ab) / 2.  At r = 3 one node joins the rest.  The state is a device
 * buffer of tracs_nj_state_bytes(n) bytes (0: n is above 2^24): the matrix (n x n f64, full symmetric), row sums and node ids per
 * slot, the join records, scratch.
 *   tracs_nj_init        the zero matrix
 *   tracs_nj_load_panel  the cells j > i of rows [row_begin, row_end) of dist / ncomp as tracs_pairsnp_dense writes them (device uint32,
 *                        indexed by ABSOLUTE row, leading dimension ld >= n), mirrored: kind 0: D_ij = d; kind 1: D_ij = d / nn
 *                        (substitutions per compared site; a cell with nn = 0 is remembered and tracs_nj_emit refuses).  ncomp may
 *                        be NULL with kind 0.  Panels may arrive in any split.
 *   tracs_nj_load_f64    the cells j > i of a device f64 matrix (leading dimension ld >= n), mirrored; the diagonal stays 0.
 *                        Both loads are one stream-ordered launch and do not synchronise; n must be the n of tracs_nj_init (a
 *                        load with another n writes nothing, and tracs_nj_run refuses the state).
 *   tracs_nj_run         the row sums (R_k = the sum of D_mk over m = 0 .. n - 1, in that order) and the n - 3 joins, enqueued on the
 *                        stream without a host read-back: per join a scan of the active triangle, the new row and row sums, and the
 *                        commit that also moves the last active slot into the retired one (the scanned block stays dense).  Once
 *                        per initialised state.  Reads the state's header first (one synchronisation of the stream, before
 *                        anything is enqueued); tracs_nj_init synchronises once as well.
 *   tracs_nj_emit        *n_joins <- max(n - 3, 0); unless NULL, the HOST arrays a, b (uint32: the joined nodes, a < b), d_ab, r_a,
 *                        r_b (double: D_ab and the two row sums when they were joined, r = n - t), room for n - 3 entries;
 *                        last_ids (HOST uint32[3]) and last_d (HOST double[3]): the last three nodes x < y < z and D_xy, D_xz, D_yz
 *                        (n = 2: the two leaves and D_01; unused entries 0xFFFFFFFF and 0).  A remembered nn = 0 cell: TRACS_E_ARG,
 *                        and zero_pair (HOST uint32[2], may be NULL; else 0xFFFFFFFF twice) receives its (i, j).  Synchronises.
 *   tracs_nj_edges       host only: branch lengths from the records, l_a = D_ab / 2 + (R_a - R_b) / (2 (r - 2)), l_b = D_ab - l_a,
 *                        for the top node l_x = ((D_xy + D_xz) - D_yz) / 2 and so on; negative lengths stay as computed.  parent,
 *                        child, length: room for 2n - 3 edges, in creation order ((n + t, a), (n + t, b) per join, then the top
 *                        node 2n - 3 with x, y, z).  n = 2: the one edge (0, 1, D_01); n < 2: none.
 *   tracs_tree_write     host only: one Newick line for those edges appended to `path` (children in the edges' order, internal
 *                        nodes unlabelled, a name with one of ()[]':;, or whitespace single-quoted with ' doubled, lengths in the
 *                        shortest decimal form that reads back to the same double; n = 2: (A:d/2,B:d/2); n = 1: A;) and, with
 *                        edges_path, the rows parent,child,length,ref appended to it, node n + t named #<t + 1>; names are written
 *                        raw there, as in every other CSV of the library (a name with a comma adds fields).  No recursion.      */
size_t tracs_nj_state_bytes(size_t n);
int tracs_nj_init(void *state, size_t n, void *stream);
int tracs_nj_load_panel(void *state, size_t n, const uint32_t *dist, const uint32_t *ncomp, size_t ld, size_t row_begin, size_t row_end,
                        int kind, void *stream);
int tracs_nj_load_f64(void *state, size_t n, const double *matrix, size_t ld, void *stream);
int tracs_nj_run(void *state, size_t n, void *stream);
int tracs_nj_emit(void *state, size_t n, size_t *n_joins, uint32_t *a, uint32_t *b, double *d_ab, double *r_a, double *r_b,
                  uint32_t *last_ids, double *last_d, uint32_t *zero_pair, void *stream);
int tracs_nj_edges(size_t n, const uint32_t *a, const uint32_t *b, const double *d_ab, const double *r_a, const double *r_b,
                   const uint32_t *last_ids, const double *last_d, uint32_t *parent, uint32_t *child, double *length, size_t *n_edges);
int tracs_tree_write(const char *const *names, size_t n, const uint32_t *parent, const uint32_t *child, const double *length,
                     size_t n_edges, const char *path, const char *ref, const char *edges_path);
/* BIONJ (Gascuel 1997; csrc/nj.hip): neighbour joining with a second matrix V of variances (V = D and RV = R at the
 * start, bit for bit) that weights every reduction.  Q, the tie rule, the record (a, b, D_ab, R_a, R_b; a the LOWER ID), the lengths,
 * the three-node end and n <= 3 are neighbour joining's; with r active nodes and one rounding per operation, bracketed as written:
 *   l_a = (0.5 D_ab) + ((R_a - R_b) / (2 (r - 2))), l_b = D_ab - l_a              (tracs_nj_edges's own operations)
 *   lambda = 0.5 if V_ab == 0, else 0.5 + ((RV_b - RV_a) / ((2 (r - 2)) V_ab)) clamped to [0, 1]; mu = 1 - lambda
 *   D_uk = (lambda (D_ak - l_a)) + (mu (D_bk - l_b));    V_uk = ((lambda V_ak) + (mu V_bk)) - ((lambda mu) V_ab)
 *   R_k <- (R_k - (D_ak + D_bk)) + D_uk;                 RV_k <- (RV_k - (V_ak + V_bk)) + V_uk
 *   R_u = (lambda ((R_a - D_ab) - ((r - 2) l_a))) + (mu ((R_b - D_ab) - ((r - 2) l_b)))
 *   RV_u = ((lambda (RV_a - V_ab)) + (mu (RV_b - V_ab))) - ((r - 2) ((lambda mu) V_ab))
 * RV_b - RV_a is Gascuel's sum over k of V_bk - V_ak (zero diagonal, symmetric V): no order-dependent reduction.  mu is rounded, so
 * the formulas are not symmetric in a and b.  Nothing is clamped but lambda: D, V and lengths may go negative.
 *   tracs_bionj_state_bytes  the bytes of a BIONJ state (0: n is above 2^24): a neighbour-joining state followed by V, RV and two
 *                            scratch rows, about 2 n^2 doubles.  A state does not record its size: as with every state of this
 *                            library the caller allocates what the method asks for.  tracs_nj_init, tracs_nj_load_panel,
 *                            tracs_nj_load_f64, tracs_nj_emit and tracs_nj_edges serve both methods (they touch the common prefix
 *                            only), and tracs_nj_run on a BIONJ-sized state runs neighbour joining.
 *   tracs_bionj_run          tracs_nj_run's contract with the BIONJ reduction: three stream-ordered launches per join, no
 *                            read-back.  The state MUST have tracs_bionj_state_bytes(n) bytes.                                     */
size_t tracs_bionj_state_bytes(size_t n);
int tracs_bionj_run(void *state, size_t n, void *stream);

/*   tracs_tree_write_changes  tracs_tree_write with a number of changes per edge (uint32[n_edges]): the Newick line is
 *                        tracs_tree_write's, byte for byte; the edge rows are parent,child,length,changes,ref.                  */
int tracs_tree_write_changes(const char *const *names, size_t n, const uint32_t *parent, const uint32_t *child, const double *length,
                             size_t n_edges, const uint32_t *changes, const char *path, const char *ref, const char *edges_path);
/*   tracs_tree_write_filtered tracs_tree_write_changes with the changes the branch filter keeps per edge (uint32[n_edges]):
 *                        the edge rows are parent,child,length,changes,filtered,ref.                                          */
int tracs_tree_write_filtered(const char *const *names, size_t n, const uint32_t *parent, const uint32_t *child, const double *length,
                              size_t n_edges, const uint32_t *changes, const uint32_t *filtered, const char *path, const char *ref,
                              const char *edges_path);

/* Bootstrap support for the neighbour-joining tree (csrc/bootstrap.hip; what tracs_distance_tree_bootstrap runs).  One
 * replicate is the run on an alignment whose L columns were drawn with replacement.  All arithmetic mod 2^64:
 *     mix(x): z = x; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
 *     G = 0x9E3779B97F4A7C15; key_b = mix(seed + G (b + 1)); u(b, t) = mix(key_b + G (t + 1)); c(b, t) = (u(b, t) L) >> 64
 * for t = 0 .. L - 1; w_b(c) = the number of t with c(b, t) = c (they sum to L).
 *   tracs_bootstrap_weights       weights (device uint32[L]) <- w_replicate.  One thread per draw, integer atomics.  Stream-ordered.
 *   tracs_alignment_gather_sites  weights: device uint32[the handle's length].  *out: a NEW handle in which column c of src is repeated
 *                                 weights[c] times, columns in ascending c, every sample: byte for byte what packing that text gives
 *                                 (pad samples, tail bits, pad groups and slack zero, N = A & C & G & T); src is left as it was.
 *                                 *n_out (may be NULL): its length, the sum of the weights.  A sum of 0 ("no column drawn") or of
 *                                 2^32 and more is refused (TRACS_E_ARG).  Synchronises the stream.
 *   tracs_tree_support            host only, no recursion: both trees as tracs_nj_edges gives them (2n - 3 edges over the same n
 *                                 leaves, in creation order).  An internal edge is one whose child is an internal node; its split is
 *                                 the set of leaves below the child, taken on the side without leaf 0 (bitsets of ceil(n / 64) words,
 *                                 built bottom-up in the edges' order).  count[e] += 1 for every internal edge e of the first tree
 *                                 whose split is the split of an internal edge of the second (a hash finds candidates, equality of
 *                                 the bitsets decides); other entries of count are left alone.  n < 4: nothing to do.
 *   tracs_tree_write_support      tracs_tree_write with support (uint32 per edge, 0xFFFFFFFF = none, else at most `replicates`): an
 *                                 internal node whose edge has one carries it as a decimal label, `(A:1,B:2)87:0.5`; the edge rows
 *                                 are parent,child,length,support,ref with NA on leaf edges and where there is none.              */
int tracs_bootstrap_weights(size_t L, uint64_t seed, uint64_t replicate, uint32_t *weights, void *stream);
int tracs_alignment_gather_sites(const tracs_alignment *src, const uint32_t *weights, tracs_alignment **out, size_t *n_out, void *stream);
int tracs_tree_support(size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges, const uint32_t *rep_parent,
                       const uint32_t *rep_child, size_t rep_n_edges, uint32_t *count);
int tracs_tree_write_support(const char *const *names, size_t n, const uint32_t *parent, const uint32_t *child, const double *length,
                             size_t n_edges, const uint32_t *support, uint32_t replicates, const char *path, const char *ref,
                             const char *edges_path);

/* Transfer bootstrap support (csrc/transfer.hip; what tracs_distance_tree_bootstrap_transfer runs; Lemoine et al.,
 * Nature 2018).  Both trees as tracs_nj_edges gives them: 2n - 3 edges over the same n leaves, in creation order, two children per
 * joined node and three at the top.  T_f: the leaves below the child of an edge f (a leaf edge: the leaf).  For an internal edge e of
 * the main tree (child >= n), S_e = T_e and p_e = min(|S_e|, n - |S_e|) >= 2.  Against one replicate tree:
 *     h(e, f) = |S_e| + |T_f| - 2 |S_e & T_f|;  delta = min(h, n - h);  phi(e) = the smallest delta over ALL 2n - 3 edges f of the replicate
 * so 0 <= phi <= p_e - 1, and phi = 0 exactly when the replicate has the split.  Over B replicates Phi_e = the integer sum of phi, and
 * the transfer support is the double 1.0 - double(Phi_e) / double(B (p_e - 1)) (the product in 64-bit integers, every step rounded to
 * nearest, computed on the host): in [0, 1], 1 = every replicate has the split, and a function of the trees alone, bit for bit.
 *   tracs_tree_transfer_program   host only, no recursion: the replicate as a post-order program of exactly 2n - 3 uint32 entries --
 *                                 a leaf l is the entry l, a joined node v the entry 0x80000000 | |T_v| after its two subtrees, the
 *                                 top node nothing; children largest subtree first (ties: lower id).  Run as "leaf: push; joined node:
 *                                 pop two, push the sum" the stack never holds more than floor(log2 n) + 3 values; *depth <- the most
 *                                 it holds.  Malformed edges are refused as tracs_tree_support refuses them.  n < 4: nothing, depth 0.
 *   tracs_transfer_state_bytes    the device state of a main tree over n leaves: a bit matrix [leaf][ceil((n - 3) / 64)] of 64-bit words
 *                                 (is the leaf in S_e), |S_e|, the sums, one program; about n^2 / 8 bytes.  0: n is too large (> 2^24).
 *   tracs_transfer_init           the main tree into the state (the matrix is built on the host and uploaded), the sums zeroed.
 *                                 Synchronises the stream.
 *   tracs_transfer_add            one replicate: its program is built and uploaded, transfer_phi_kernel (one lane per internal edge of
 *                                 the main tree, one wave per 64) adds phi to every sum.  phi: NULL, or DEVICE uint32[2n - 3] that
 *                                 receives this replicate's phi at the internal edges (other entries are left alone).  The kernel is
 *                                 stream-ordered.  n < 4: nothing.
 *   tracs_transfer_emit           sum_phi (host uint64 per edge) <- Phi_e, light (host uint32 per edge) <- p_e at the internal edges of
 *                                 the main tree; entries of leaf edges are left alone; either may be NULL.  n < 4: nothing.
 *   tracs_tree_transfer           the one-shot sibling of tracs_tree_support: host arrays, a state of its own, init + add; phi (host
 *                                 uint32 per edge of the first tree) <- phi at its internal edges, other entries left alone.
 *   tracs_tree_write_transfer     tracs_tree_write_support with the transfer support as the label, in the shortest decimal form that
 *                                 reads back to the same double (as the lengths): `(A:1,B:2)0.875:0.5`; the edge rows are
 *                                 parent,child,length,support,transfer,ref, both NA on leaf edges.  n < 4: no labels, NA.       */
int tracs_tree_transfer_program(size_t n, const uint32_t *rep_parent, const uint32_t *rep_child, size_t n_edges, uint32_t *program,
                                size_t *depth);
size_t tracs_transfer_state_bytes(size_t n);
int tracs_transfer_init(void *state, size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges, void *stream);
int tracs_transfer_add(void *state, size_t n, const uint32_t *rep_parent, const uint32_t *rep_child, size_t rep_n_edges, uint32_t *phi,
                       void *stream);
int tracs_transfer_emit(void *state, size_t n, uint64_t *sum_phi, uint32_t *light);
int tracs_tree_transfer(size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges, const uint32_t *rep_parent,
                        const uint32_t *rep_child, size_t rep_n_edges, uint32_t *phi);
int tracs_tree_write_transfer(const char *const *names, size_t n, const uint32_t *parent, const uint32_t *child, const double *length,
                              size_t n_edges, const uint32_t *support, const uint64_t *sum_phi, const uint32_t *light, uint32_t replicates,
                              const char *path, const char *ref, const char *edges_path);

/* Histogram of pair values over dense panels (csrc/histogram.hip; what tracs_distance_histogram runs).  The state is
 * a device buffer of tracs_hist_state_bytes(n_bins) bytes: per value v in [0, n_bins) three 64-bit counts -- pairs `within` a group
 * (both samples grouped, equal labels), `between` groups (both grouped, labels differ) and `ungrouped` (a sample with label < 0, or
 * group == NULL) -- plus a count of offered values >= n_bins.  group: device int32[n], or NULL.  Counts are exact; the state is a
 * sum, so it does not depend on how the pairs are split into updates.  1 <= n_bins <= 2^31 (else TRACS_E_ARG; _state_bytes: 0).
 *   tracs_hist_init        every count 0
 *   tracs_hist_update      count the cells of tracs_pairsnp_dense[_thr] in the panel rows [row_begin, row_end): columns
 *                          j >= max(col_begin, i + 1), indexed by ABSOLUTE row, leading dimension ld, n < 2^30.  A cell is counted
 *                          iff it is, read as unsigned, <= dist_threshold (tracs_coo_count's rule).  One launch, the panel read once.
 *   tracs_hist_update_coo  count m listed pairs (rows[t], cols[t]) (device uint32; only read with group != NULL) with value val[t]
 *   tracs_hist_emit        *n_rows <- the non-empty bins; unless all four are NULL, value (device uint32) and within / between /
 *                          ungrouped (device uint64), room for *n_rows entries each (ask with NULLs first), receive them ascending
 *                          by value.  Fails with a message when a value >= n_bins was offered.  Synchronises the stream.          */
size_t tracs_hist_state_bytes(size_t n_bins);
int tracs_hist_init(void *state, size_t n_bins, void *stream);
int tracs_hist_update(const uint32_t *dist, size_t ld, size_t n, size_t row_begin, size_t row_end, size_t col_begin,
                      int32_t dist_threshold, const int32_t *group, void *state, size_t n_bins, void *stream);
int tracs_hist_update_coo(const uint32_t *rows, const uint32_t *cols, const uint32_t *val, size_t m, const int32_t *group,
                          void *state, size_t n_bins, void *stream);
int tracs_hist_emit(void *state, size_t n_bins, size_t *n_rows, uint32_t *value, uint64_t *within, uint64_t *between,
                    uint64_t *ungrouped, void *stream);

/* Recombination filter (src/pairsnp.hpp:251-318) on emitted pairs.  rows/cols: device uint32[n_pairs];
 * pos_off: device int64[n_pairs+1] = exclusive scan of the pairs' SNP distances; positions: device uint32
 * workspace of pos_off[n_pairs] entries (receives each pair's sorted SNP sites); found[t] = SNP bits seen
 * (equals the distance); filt[t] = filtered distance.                                                  */
int tracs_filter_recomb_device(const tracs_alignment *a, const uint32_t *rows, const uint32_t *cols, size_t n_pairs,
                               const int64_t *pos_off, uint32_t *positions, uint32_t *found, uint32_t *filt,
                               void *stream);

/* The same filter without the positions (what `tracs distance --filter` and tracs_pairsnp(filter = 1) use): filt[t] =
 * filter_recomb (src/pairsnp.hpp:251-318) of the emitted pair (rows[t], cols[t]) whose SNP distance is d[t] (:405-413); all
 * device uint32[n_pairs].  A pair's SNP sites come from the two samples' departure lists (the sites at which a sample is neither
 * N nor exactly the site's reference base), built with two N bitmaps once per packed alignment and kept on the handle; pairs
 * whose lists do not fit a wave's LDS, and alignments too divergent for lists, are scanned like the reference scans them.
 * TRACS_FILTER_LISTS=0: always the scan; TRACS_FILTER_TABLE=0: the binomial tail summed per SNP instead of per distinct
 * (d, count).  Synchronises the stream (an internal consistency check: every pair's SNP count must equal d[t]).            */
int tracs_filter_recomb_pairs(tracs_alignment *a, const uint32_t *rows, const uint32_t *cols, const uint32_t *d, size_t n_pairs,
                              uint32_t *filt, void *stream);

/* The SNP sites of listed pairs (csrc/pair_sites.hip): what tracs_pairsnp_dense counts and the filter sums, kept
 * per site.  rows / cols: device uint32[n_pairs], sample indices in either order; a pair may repeat.  No distance is supplied.
 *   tracs_pair_sites_count  d[t] (device uint32[n_pairs]) = the sites at which the two samples' allele sets are disjoint
 *                           (src/pairsnp.hpp:398-403); off (device int64[n_pairs + 1]) = the exclusive scan of d; *total (host) =
 *                           off[n_pairs].  An index >= n is refused (TRACS_E_ARG).  Synchronises the stream.
 *   tracs_pair_sites_fill   the entries of pair t at site / info [off[t] - entry_base, off[t + 1] - entry_base) (device uint32, room
 *                           entries each; nothing is stored outside [0, room)), ascending by site: site = the index into the packed
 *                           alignment (the kept columns), info = the rows[t] sample's allele mask in bits 0-3 and the cols[t]
 *                           sample's in bits 4-7 (A = 1, C = 2, G = 4, T = 8; neither is 15).  filter != 0: bit 8 is set on the SNPs
 *                           filter_recomb drops (src/pairsnp.hpp:251-318: with d <= 1 none; else those whose window holds more than
 *                           one SNP and has 1 - CDF < 0.05 / d), so the entries without it number tracs_filter_recomb_pairs' filt[t].
 *                           A subrange of the pairs is filled by passing rows + t0, cols + t0, off + t0 and entry_base = off[t0].
 * TRACS_PAIR_SITES_LANES_MIN (diagnostic): the number of pairs from which count and fill take a pair per lane instead of a wave per
 * pair (default 16 384, as TRACS_FILTER_LANES_MIN).                                                                              */
int tracs_pair_sites_count(const tracs_alignment *a, const uint32_t *rows, const uint32_t *cols, size_t n_pairs, uint32_t *d, int64_t *off,
                           uint64_t *total, void *stream);
int tracs_pair_sites_fill(const tracs_alignment *a, const uint32_t *rows, const uint32_t *cols, size_t n_pairs, const int64_t *off,
                          int64_t entry_base, uint32_t *site, uint32_t *info, size_t room, int filter, void *stream);

/* Every site placed on a fixed tree: small parsimony, Fitch's two passes (csrc/fitch.hip; not in the reference).  The
 * alignment's sample i has the mask m_i(s) at site s (A = 1, C = 2, G = 4, T = 8; N = 15).  parent / child: HOST uint32[n_edges], the
 * tree exactly as tracs_nj_edges gives it for the alignment's n samples -- 2n - 3 edges in creation order, (n + t, a_t), (n + t, b_t)
 * with a_t < b_t for join t = 0 .. n - 4, then the top node T = 2n - 3 with x < y < z (n = 2: the edge (0, 1); n = 1: none) --
 * anything else is refused (TRACS_E_ARG) before a launch.  Per site, independently:
 *     bottom-up, ascending node id: S_i = m_i for a leaf; join: I = S_a & S_b, S = I if I != 0, else S_a | S_b; top node: S_xy by
 *         the same rule, then I = S_xy & S_z, S_T = I if I != 0, else S_xy
 *     top-down: f_T = lowbit(S_T) (A before C before G before T); the edges by descending parent id, creation order within a parent;
 *         f_child = f_parent if f_parent & S_child != 0, else lowbit(S_child); a CHANGE is an edge with f_child != f_parent
 *     n = 2: f_0 = lowbit(m_0 & m_1), or lowbit(m_0) where that is empty; f_1 by the child rule (the changes number d(0, 1))
 *     minimum(s) = (the smallest |H|, H a non-empty set of bases with m_i(s) & H != 0 for every i) - 1
 * A leaf's state lies in its mask; an N leaf copies its parent; the number of changes of a site is its parsimony length on this tree
 * (unique); their placement is ONE most-parsimonious reconstruction among possibly several.
 *   tracs_fitch_count  device outputs: edge_changes uint32[n_edges], site_changes uint32[L], site_minimum uint8[L], off int64[L + 1] =
 *                      the exclusive scan of site_changes; *total (host) = off[L].  Synchronises the stream.
 *   tracs_fitch_fill   the entries of the sites [site_begin, site_end): those of site s at site / edge / info
 *                      [off[s] - entry_base, off[s + 1] - entry_base) (device uint32, room entries each; nothing is stored outside
 *                      [0, room)), in the order of the top-down walk (ancestors before descendants): site = the index into the packed
 *                      alignment, edge = the index into the edge list, info = f_parent in bits 0-3 and f_child in bits 4-7, both
 *                      one-hot.  Deterministic: no atomic decides a position.
 * The sets of all nodes live in a workspace buffer for a slab of sites at a time, sized from a byte budget;
 * TRACS_FITCH_SLAB_GROUPS (diagnostic): the slab's length in groups of 128 sites.                                                  */
int tracs_fitch_count(const tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, uint32_t *edge_changes,
                      uint32_t *site_changes, uint8_t *site_minimum, int64_t *off, uint64_t *total, void *stream);
int tracs_fitch_fill(const tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, size_t site_begin, size_t site_end,
                     const int64_t *off, int64_t entry_base, uint32_t *site, uint32_t *edge, uint32_t *info, size_t room, void *stream);

/* The recombination filter on the tree's branches (csrc/fitch.hip, csrc/filter_lists.hip; not in the reference).  The
 * input is the packed alignment with its L sites in packed coordinates, exactly as the pair filter sees them, together with the tree
 * and its Fitch reconstruction as defined above.
 *     For edge e, C_e is the ascending list of the sites with a change on e and d_e = |C_e| (edge_changes[e] of tracs_fitch_count).
 *     kept_e = filter_recomb(C_e, d_e, L) (src/pairsnp.hpp:251-318): d_e <= 1: everything is kept.  Otherwise p = d_e / L, the
 *     threshold is 0.05 / d_e and the half window wh = clamp(int(1 / p / 2 + 1), 50, 5000).  A change at site s is DROPPED iff its
 *     window [max(0, s - wh), min(L, s + wh + 1)) holds count > 1 changes of that edge, spanning `length` sites first to last, with
 *     1 - BinomCDF(count; length, p) < 0.05 / d_e (count >= length: CDF = 1).  kept_e is the number of changes not dropped.
 * Nothing else moves: the tree is built from the unfiltered distances and the filter is not iterated into the topology; the verdicts
 * belong to the one reconstruction that the top-down pass picks.  An N leaf never carries a change, so it never carries a drop.
 *   tracs_fitch_edge_sites    the changes regrouped by edge.  parent / child as above (HOST), edge_changes: tracs_fitch_count's (device).
 *                             edge_off (device int64[n_edges + 1]) <- the exclusive scan of edge_changes; edge_site (device uint32[room])
 *                             <- the sites of edge e at [edge_off[e], edge_off[e + 1]), ASCENDING; nothing is stored outside [0, room).
 *                             Deterministic: no atomic decides a position -- the walk stores a wave's count per (chunk of 2 048 sites,
 *                             edge), a column scan makes them bases, and the walk again places every change.  The [chunk][edge] matrix
 *                             holds a range of sites at a time (256 MiB; TRACS_FITCH_MATRIX_CHUNKS: chunks per range, diagnostic).
 *   tracs_filter_recomb_lists the window test on n_lists sorted lists (device): list t is pos[off[t] .. off[t + 1]), off int64[n_lists + 1]
 *                             with off[0] = 0, pos uint32[n_entries].  filt[t] (device uint32[n_lists]) <- the entries kept, with L =
 *                             a->L; dropped (device uint8[n_entries], or NULL) <- 1 on the entries dropped, 0 on the others.  Every
 *                             list MUST be ascending and below L: that is not checked.  Offsets that decrease, or that end beyond
 *                             n_entries, are refused (TRACS_E_ARG) before a launch.  The verdicts come from the same threshold rows
 *                             and the same tail sum as tracs_filter_recomb_pairs's (rows kept on the handle; TRACS_FILTER_TABLE=0:
 *                             the sum per entry); the departure lists of the pair routes are neither needed nor built.
 *   tracs_fitch_mark_dropped  bit 8 of info (the bit tracs_pair_sites_fill sets with filter != 0) on the entries of a batch that
 *                             tracs_fitch_fill filled and that `dropped` marks: entry k = (site[k], edge[k]) is looked up in its
 *                             edge's segment of edge_site.  All arrays on the device.                                             */
int tracs_fitch_edge_sites(const tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, const uint32_t *edge_changes,
                           int64_t *edge_off, uint32_t *edge_site, size_t room, void *stream);
int tracs_filter_recomb_lists(tracs_alignment *a, const int64_t *off, const uint32_t *pos, size_t n_lists, size_t n_entries, uint32_t *filt,
                              uint8_t *dropped, void *stream);
int tracs_fitch_mark_dropped(const uint32_t *site, const uint32_t *edge, uint32_t *info, size_t n_entries, size_t n_edges, const int64_t *edge_off,
                             const uint32_t *edge_site, const uint8_t *dropped, void *stream);

/* The branch filter's verdicts turned back into an alignment (csrc/tree_mask.hip; not in the reference): what one
 * iteration of tracs_distance_tree_iterate masks.
 *   tracs_alignment_clone          *out: a NEW handle with src's n, L and planes, byte for byte (a device-to-device copy; no existing
 *                                  entry gives one: tracs_alignment_select_sites and _gather_sites re-pack through a gather); src is left
 *                                  as it was.  A copy that does not fit in the device's memory is refused (TRACS_E_NOMEM) with a message
 *                                  that says so.  Stream-ordered.
 *   tracs_alignment_restore        dst's planes <- src's, the same copy into an existing handle of src's n and L (anything else is
 *                                  refused): what tracs_distance_tree_iterate does to its clone between iterations.  It counts as a
 *                                  re-pack of dst.  Stream-ordered.
 *   tracs_alignment_mask_subtrees  parent / child: HOST uint32[n_edges], the tree exactly as tracs_fitch_count takes it for a's n samples;
 *                                  anything else is refused (TRACS_E_ARG) before a launch.  edge_off (device int64[n_edges + 1]),
 *                                  edge_site (device uint32[n_entries]) and dropped (device uint8[n_entries]): what
 *                                  tracs_fitch_edge_sites and tracs_filter_recomb_lists leave.  Offsets that do not start at 0, that
 *                                  decrease, or that end beyond n_entries are refused before a launch.  For every entry k of edge e
 *                                  with dropped[k] != 0 and every sample i below e (the leaves in the subtree of e's child, the side away
 *                                  from the top node; n = 2: the sample 1) the cell (i, edge_site[k]) becomes N: the site's bit is
 *                                  set in the four allele planes and the N plane.  The host derives a leaf order (depth-first from the
 *                                  top node) in which every edge's leaves are an interval; the device gives every entry the weight
 *                                  |below(e)| or 0, scans the weights (the total W is 64-bit and is run over in ranges) and takes one
 *                                  (entry, leaf) cell per lane with an atomic OR per plane word.  An entry with site >= L stores
 *                                  nothing; tail bits and pad samples stay 0.  *n_cells (may be NULL) <- the cells that were not N and
 *                                  now are (a set, so deterministic).  Masking counts as a re-pack of `a`: what the handle caches per
 *                                  pack is rebuilt by the next call.  Synchronises the stream.                                       */
int tracs_alignment_clone(const tracs_alignment *src, tracs_alignment **out, void *stream);
int tracs_alignment_restore(tracs_alignment *dst, const tracs_alignment *src, void *stream);
int tracs_alignment_mask_subtrees(tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, const int64_t *edge_off,
                                  const uint32_t *edge_site, const uint8_t *dropped, size_t n_entries, uint64_t *n_cells, void *stream);

/* transcluster on device arrays (same math as tracs_trans_dist).  workspace is managed
 * internally (hipMallocAsync on the stream).  exp_p0 != 0 writes exp(p0) (what
 * tracs/transcluster.py:38-39 returns with log=False).                                     */
int tracs_trans_dist_device(const int32_t *snpdiff, const double *datediff, size_t n, double lamb,
                            double beta, double threshold_Ek, int exp_p0, double *p0, double *eK,
                            void *stream);
/* Dense variant used by the distance pipeline: for the same cell set as tracs_pairsnp_dense,
 * delta(i,j) = |day_i - day_j| * 86400 / 31556952.0  (tracs/transcluster.py:5,26-33), N = dist[i*ld+j];
 * writes p0[i*ld+j] (exp'ed if exp_p0) and eK[i*ld+j].  Cells with dist > dist_threshold are skipped. */
int tracs_trans_dist_dense(const uint32_t *dist, size_t ld, size_t n, size_t row_begin, size_t row_end,
                           size_t col_begin, int32_t dist_threshold, const int32_t *days, double lamb,
                           double beta, double threshold_Ek, int exp_p0, double *p0, double *eK,
                           void *stream);

/* Same over one or two row panels [b0,e0) (, [b1,e1)) in ONE pass (one key table): row_ranges = {b0,e0[,b1,e1]}. */
int tracs_trans_dist_dense2(const uint32_t *dist, size_t ld, size_t n, const size_t *row_ranges, int n_ranges,
                            size_t col_begin, int32_t dist_threshold, const int32_t *days, double lamb, double beta,
                            double threshold_Ek, int exp_p0, double *p0, double *eK, void *stream);

/* Multi-GPU form of the dense variant: the distinct (N, day gap) keys of the cells are evaluated into a dense key
 * table [n_max + 1][d_max + 1] (device f64, zeroed by the caller; log p0 and E(K)); a rank evaluates only the keys of its hash
 * class `part` of `parts`, the caller all-reduces (sums) the tables over the ranks, and tracs_trans_table_gather then writes
 * p0 / eK of every cell from the completed table.  *overflow (device uint32, zeroed by the caller) is set if a key falls
 * outside the table.  Same arithmetic as tracs_trans_dist_dense.                                                       */
int tracs_trans_table_dense(const uint32_t *dist, size_t ld, size_t n, size_t row_begin, size_t row_end, size_t col_begin,
                            int32_t dist_threshold, const int32_t *days, double lamb, double beta, double threshold_Ek,
                            int part, int parts, uint32_t n_max, uint32_t d_max, double *table_p0, double *table_eK,
                            uint32_t *overflow, void *stream);
int tracs_trans_table_gather(const uint32_t *dist, size_t ld, size_t n, size_t row_begin, size_t row_end, size_t col_begin,
                             int32_t dist_threshold, const int32_t *days, uint32_t n_max, uint32_t d_max,
                             const double *table_p0, const double *table_eK, int exp_p0, double *p0, double *eK,
                             uint32_t *overflow, void *stream);

/* The distinct keys SPLIT over ranks that each hold rows of the matrix (site shards): src/transcluster.hpp:245-246,
 * 265-282 memoises per (N, delta) key -- here every key of the WHOLE matrix is evaluated by exactly one rank.
 *   tracs_trans_keys_words     uint32 words of a key bitmap (the (N, day gap) grid + four words: largest distance, smallest and
 *                              largest day + 2^31, "a key fell outside the grid")
 *   tracs_trans_keys_mark      the keys of the cells (i in the row ranges -- 0, 1 or 2 --, j >= max(col_begin, i + 1), d <=
 *                              dist_threshold) marked into `keys` (device, tracs_trans_keys_words() words, overwritten)
 *   tracs_trans_keys_merge     keys <- the union of `parts` bitmaps laid end to end in `all` (what an all-gather leaves)
 *   tracs_trans_keys_info      host info[4] = {distinct keys, largest distance, span of the days, 1 if the keys fit the grid};
 *                              synchronises the stream.  info[3] == 0: take tracs_trans_dist_dense2 on the own rows instead
 *   tracs_trans_keys_evaluate  the keys whose ordinal (set bits before it in the union) is = part mod parts, evaluated into
 *                              vals[2 (ordinal / parts)] = log p0, [.. + 1] = E(K) (device f64, per >= ceil(keys / parts) slots)
 *   tracs_trans_keys_gather    vals_all = the `parts` arrays of `per` slots each, end to end (what an all-gather leaves): p0 / eK
 *                              of every cell of the row ranges, as tracs_trans_dist_dense2 writes them
 * Same arithmetic per key as tracs_trans_dist_dense.                                                                          */
size_t tracs_trans_keys_words(void);
int tracs_trans_keys_mark(const uint32_t *dist, size_t ld, size_t n, const size_t *row_ranges, int n_ranges, size_t col_begin,
                          int32_t dist_threshold, const int32_t *days, uint32_t *keys, void *stream);
int tracs_trans_keys_merge(uint32_t *keys, const uint32_t *all, int parts, void *stream);
int tracs_trans_keys_info(const uint32_t *keys, uint64_t *info, void *stream);
int tracs_trans_keys_evaluate(const uint32_t *keys, const uint64_t *info, int part, int parts, double lamb, double beta,
                              double threshold_Ek, double *vals, size_t per, void *stream);
int tracs_trans_keys_gather(const uint32_t *dist, size_t ld, size_t n, const size_t *row_ranges, int n_ranges, size_t col_begin,
                            int32_t dist_threshold, const int32_t *days, const uint32_t *keys, const uint64_t *info,
                            const double *vals_all, int parts, size_t per, int exp_p0, double *p0, double *eK, void *stream);

/* calculate_posteriors on device arrays; counts/posterior are device f64 [L][K].            */
int tracs_calculate_posteriors_device(const double *counts, size_t L, size_t K, const double *alphas_host,
                                      int keep, double threshold, double *posterior, void *stream);
/* Fused production form (config 4): uint16 counts [L][4] -> 4-bit allele mask per site
 * (bit0=A..bit3=T set where posterior > 0, i.e. what tracs/align.py:616-622 turns into an
 * IUPAC letter), two sites per output byte (low nibble = even site).                        */
int tracs_posterior_codes_device(const uint16_t *counts, size_t L, const double *alphas_host, int keep,
                                 double threshold, uint8_t *codes, void *stream);

int tracs_find_dirichlet_priors_device(const double *counts, size_t L, size_t K, int max_iter, double tol, int method,
                                       double error_filt_threshold, double *alphas_out_host, int *iters_out,
                                       void *stream);
/* Tests only: the digamma the fit sums (csrc/dirichlet.hip digamma_pos), evaluated on the device for n host doubles > 0.  */
int tracs_debug_digamma(const double *x, size_t n, double *out);
/* Tests only: the contents of memory the library should not be reading, as a controlled input.
 *   tracs_debug_poison_scratch(byte)   0 .. 255: on; -1 (the default; any other value too): off.  While on, every OUTERMOST entry-point
 *                                      call that uses the scratch pool (an entry point that calls another one counts once: what the
 *                                      outer call holds is left alone) first drains the device, fills every allocated scratch slot
 *                                      of its device with `byte` and drains again; a slot allocated or regrown inside a call is
 *                                      filled before it is handed out.  Nothing in a slot survives from one entry-point call to the
 *                                      next -- which is the library's contract for its scratch anyway: results are the same with
 *                                      poison on, only slower.  (The one reader of scratch outside a call is a diagnostic this header
 *                                      does not declare, tracs_debug_trans_routes in csrc/transcluster.hip: the counters of the last
 *                                      key evaluation, valid only until the next entry-point call; the contract is at its definition.)  Off costs one untaken branch per call.  Caller-owned states, outputs
 *                                      and what a tracs_alignment caches are not touched.  Process-wide; not meant to be switched
 *                                      while another thread is inside the library.
 *   tracs_debug_scratch_hits(hits, n)  returns the number of scratch slots S; hits[s] (s < min(n, S); hits may be NULL) <- how often
 *                                      slot s has been handed out, by any device, since the previous call of this function.  Every
 *                                      count is then reset to zero.  Slots are numbered as csrc/common.h's enum WsSlot.             */
void tracs_debug_poison_scratch(int byte);
size_t tracs_debug_scratch_hits(uint64_t *hits, size_t room);

/* The same with the align stage's coverage rules (tracs/align.py:599-613): sites with total count < min_cov, or with
 * cov_lo <= total <= cov_hi (outlier band; pass cov_lo > cov_hi to disable), become fully ambiguous (mask 15).        */
int tracs_posterior_codes_cov_device(const uint16_t *counts, size_t L, const double *alphas_host, int keep,
                                     double threshold, uint32_t min_cov, double cov_lo, double cov_hi, uint8_t *codes,
                                     void *stream);
/* Align stage before the posterior filter (tracs/align.py:473-516): one pass over device f64 counts [L][4] that
 *   - histograms the per-site coverage rs = A+C+G+T into hist[min(rs, nbins-1)] (device uint64[nbins], zeroed here): the
 *     stage's statistics (fraction covered, fraction >= min_cov, np.median / np.quantile of the non-zero coverages,
 *     :476-480,522,559) are order statistics of it;
 *   - narrows the counts to uint16 [L][4] (counts16, may be NULL) for the two code kernels;
 *   - sets *bad (device uint32) if any count is not an integer in [0, 65535].                                          */
int tracs_coverage_profile_device(const double *counts, size_t L, uint64_t *hist, size_t nbins, uint16_t *counts16,
                                  uint32_t *bad, void *stream);
/* --consensus calls (tracs/align.py:482-493): mask = the first allele with the largest count; 15 (N) where the total
 * count is below min_cov.  Same packed 4-bit output as tracs_posterior_codes_device.                                   */
int tracs_consensus_codes_device(const uint16_t *counts16, size_t L, uint32_t min_cov, uint8_t *codes, void *stream);
/* The three entry points above for per-allele counts beyond 65535 (deep amplicon / viral data; the reference works on
 * float64 counts of any depth, tracs/align.py:444-647): uint32 counts [L][4], each < 2^30.  The coverage histogram's last
 * bin then collects every total >= nbins - 1; callers needing order statistics up there take them from the counts.      */
int tracs_coverage_profile_device32(const double *counts, size_t L, uint64_t *hist, size_t nbins, uint32_t *counts32,
                                    uint32_t *bad, void *stream);
int tracs_posterior_codes_cov_device32(const uint32_t *counts, size_t L, const double *alphas_host, int keep,
                                       double threshold, uint32_t min_cov, double cov_lo, double cov_hi, uint8_t *codes,
                                       void *stream);
int tracs_consensus_codes_device32(const uint32_t *counts32, size_t L, uint32_t min_cov, uint8_t *codes, void *stream);
/* 4-bit masks -> IUPAC letters as tracs/align.py:285-323,616-622 ('X' for mask 0, 'N' for 15); ascii: device, L bytes. */
int tracs_codes_to_iupac_device(const uint8_t *codes, size_t L, uint8_t *ascii, void *stream);
/* Pack ONE sample straight from its 4-bit masks (no FASTA round trip): mask 0 ('X') is treated like every other
 * non-IUPAC letter, i.e. fully ambiguous (src/pairsnp.hpp:192-197).  codes: device, (L+1)/2 bytes.                   */
int tracs_alignment_pack_codes(tracs_alignment *a, const uint8_t *codes, size_t sample, void *stream);
/* The same for `count` samples [first, first+count) in one launch: sample k's masks start at codes + k * stride_bytes
 * (stride_bytes >= (L+1)/2; a multiple of 16 lets the kernel use 16-byte loads).                                       */
int tracs_alignment_pack_codes_batch(tracs_alignment *a, const uint8_t *codes, size_t stride_bytes, size_t first,
                                     size_t count, void *stream);

/* Connected components on device edge arrays; labels as tracs_connected_components.         */
int tracs_connected_components_device(const int32_t *I, const int32_t *J, size_t n_edges, size_t n_nodes,
                                      int32_t *labels, int32_t *n_components_host, void *stream);

/* ===================================================================================== */
/* (3) ON-DISK FORMATS either side of the path (host side)            */
/* ===================================================================================== */

/* `htsbox pileup -C -s 0` text (plain or gzip) -> allele counts, the parse loop of tracs/align.py:452-472.
 *   Per line: fields split at whitespace; contig = field 0, 1-based position = field 1, reference base = field 2,
 *   alleles = second-to-last field split at ',', strand counts = last field split at ':' (pieces 1 and 2, each split
 *   at ','); count[A|C|G|T] = forward + reverse for alleles that are exactly A/C/G/T when the reference base is one
 *   too; with require_both_strands an allele seen on one strand only counts 0; a repeated position overwrites.
 *   counts: host [sum(contig_lengths)][4] f64 in contig order (np.concatenate at :473), zeroed here first.
 *   Unknown contig, position outside its contig or a non-integer field is an error (the reference raises).      */
int tracs_pileup_counts(const char *path, const char *const *contig_names, const uint64_t *contig_lengths,
                        size_t n_contigs, int require_both_strands, double *counts, uint64_t *n_lines_out);

/* posterior [L][K] f64 -> gzip CSV exactly as np.savetxt(fmt="%0.5f", delimiter=",") + the trailing "\n" the
 * reference appends (tracs/align.py:580-596).  gzip_level 0..9.                                                   */
int tracs_write_posterior_csv(const char *path, const double *post, size_t L, size_t K, int gzip_level);

/* Starts, on a thread of its own, what a process's first call otherwise waits for: the HIP runtime, the device context and this
 * library's code object.  Returns at once; later calls wait where they need the device.  `tracs distance` calls it before it reads
 * its metadata (tracs/distance.py:161-166) -- a 10 x 100 kb alignment spends more time starting up than computing.  No-op unless
 * exactly one device is visible. */
void tracs_warm_up(void);

/* `tracs distance` for one alignment (tracs/distance.py:159-258) with the results on the device until the CSV rows.
 *   tracs_distance_open   read + pack the FASTA file(s) (1 file: all pairs; 2: file 0 x file 1, src/pairsnp.hpp:348-360); the names
 *                         (tracs_distance_nseq / _name) are what the caller looks the sampling dates up by
 *   tracs_distance_run    row panel by row panel: tracs_pairsnp_dense_thr, tracs_trans_dist_dense when `days` (host, one whole day
 *                         number per sample: delta = |day_i - day_j| x 86400 / 31556952.0 years, tracs/transcluster.py:26-33) is
 *                         given, COO extraction incl. P(direct) and E(K), one device-to-host pass in batches, rows formatted and
 *                         appended to `path` (the caller has written the header) in the reference's format and order.  days == NULL:
 *                         no metadata ("NA" for delta / P / E(K), 0 in the filtered column, :240-258); else "NA" in the filtered
 *                         column (:204) and, k_max >= 0, only rows with k_max >= E(K) (:222).  filter != 0 (--filter): the emitted
 *                         pairs go through tracs_filter_recomb_pairs (src/pairsnp.hpp:405-413), the filtered column holds their
 *                         filtered distances, and P(direct) / E(K) are those of the FILTERED distance (tracs/distance.py:183-193),
 *                         evaluated per emitted pair (tracs_trans_dist_device) instead of on the panel.                          */
typedef struct tracs_distance tracs_distance;
int tracs_distance_open(const char *const *fasta, int n_fasta, tracs_distance **out);
/*   tracs_distance_open_sites  tracs_distance_open under a site rule (tracs_alignment_select_sites' keep / keep_len / max_n_samples):
 *                         every later call on the handle sees the kept columns only.  _source_len: columns read; _len: columns kept;
 *                         _kept_sites: the final bitmap over the columns read, ceil(source_len / 64) host words.                  */
int tracs_distance_open_sites(const char *const *fasta, int n_fasta, const uint64_t *keep, size_t keep_len, uint32_t max_n_samples,
                              tracs_distance **out);
/*   tracs_distance_open_rules  tracs_distance_open under a tracs_rules: every later call on the handle sees the surviving samples
 *                         (tracs_distance_nseq / _name) and the kept columns only, and _run, _forest and _histogram apply the handle's
 *                         min_sites to every dense panel before anything reads it.  _source_nseq / _source_name / _source_n_count /
 *                         _source_kept / _rule_sites: as the tracs_pairsnp_source_* accessors.                                      */
int tracs_distance_open_rules(const char *const *fasta, int n_fasta, const tracs_rules *rules, tracs_distance **out);
size_t tracs_distance_source_nseq(const tracs_distance *h);
const char *tracs_distance_source_name(const tracs_distance *h, size_t i);
uint32_t tracs_distance_source_n_count(const tracs_distance *h, size_t i);
int tracs_distance_source_kept(const tracs_distance *h, size_t i);
size_t tracs_distance_rule_sites(const tracs_distance *h);
size_t tracs_distance_source_len(const tracs_distance *h);
size_t tracs_distance_len(const tracs_distance *h);
int tracs_distance_kept_sites(const tracs_distance *h, uint64_t *kept);
size_t tracs_distance_nseq(const tracs_distance *h);
const char *tracs_distance_name(const tracs_distance *h, size_t i);
int tracs_distance_run(tracs_distance *h, int dist, const int32_t *days, double lamb, double beta, double precision, double k_max,
                       const char *path, const char *ref, int filter, uint64_t *rows_written, uint64_t *n_pairs);
/*   tracs_distance_forest `--mst WEIGHT` (not in the reference): the pairs tracs_distance_run would write (d <= dist;
 *                         k_max >= 0 with days: k_max >= E(K)) are eligible; only their minimum spanning forest (tracs_msf_*) under
 *                         weight 0: d, 1: the filtered d (filter != 0), 2: P(direct), 3: E(K) (2, 3: days != NULL) is appended to
 *                         `path`, in (i, j) order, each row byte-identical to tracs_distance_run's.  n_eligible: the eligible pairs. */
int tracs_distance_forest(tracs_distance *h, int dist, const int32_t *days, double lamb, double beta, double precision, double k_max,
                          int filter, int weight, const char *path, const char *ref, uint64_t *rows_written, uint64_t *n_eligible);
/*   tracs_distance_ancestors `--ancestors WEIGHT` (not in the reference): tracs_distance_forest's panel loop with
 *                         tracs_anc_update_coo in place of the forest update.  days (HOST int32[n], required) order the samples; each
 *                         sample's source is chosen among the pairs tracs_distance_run would write, under weight 0: d, 1: the
 *                         filtered d (filter != 0), 3: E(K), all ascending, or 2: P(direct) DESCENDING (the likeliest source first;
 *                         tracs_distance_forest's weight 2 is ascending).  The chosen pairs' rows are appended to `path` in (i, j)
 *                         order, each byte-identical to tracs_distance_run's.  tree_path != NULL: one line per sample is appended to
 *                         it, in order: sample,date,ancestor,ancestor date,root,generation,ref -- meta_dates[s] (n strings, required
 *                         then) is sample s's date as text; a root has empty ancestor fields, itself as root and generation 0.
 *                         n_eligible: the candidates offered (eligible pairs with unequal days).                                */
int tracs_distance_ancestors(tracs_distance *h, int dist, const int32_t *days, double lamb, double beta, double precision, double k_max,
                             int filter, int weight, const char *path, const char *ref, const char *tree_path,
                             const char *const *meta_dates, uint64_t *rows_written, uint64_t *n_eligible);
/*   tracs_distance_tree_run `--tree nj` and everything behind it (not in the reference): one request, one
 *                         result, one body.  The main tree: the neighbour-joining tree (tracs_nj_*) of the handle's samples, one
 *                         alignment (no second file).  The panel walk without a threshold and without the pair rule; every panel is
 *                         loaded into the matrix (kind 0: SNP distances, 1: per compared site -- a pair compared over 0 sites is
 *                         refused by name), the joins run on the device, lengths are computed on the host.  One Newick line is
 *                         appended to `path`; edges_path != NULL: the 2n - 3 rows parent,child,length,..,ref are appended to it.
 *                         Then at most one of two stages; a request with both is refused.
 *                         replicates >= 1 (`--bootstrap B`; kind 0 only): bootstrap replicates b = 0 .. replicates - 1
 *                         under `seed`: the columns at which two samples differ are selected once (the others add nothing to any
 *                         replicate's distances), and per replicate the draws are counted over them, the replicate is gathered
 *                         into a handle of its own (tracs_alignment_gather_sites; none drawn: the zero matrix), the same panel
 *                         walk, load, joins and lengths give its tree, tracs_tree_support counts its splits, and the handle is
 *                         freed.  The Newick line carries the counts as labels and the edge rows a support field
 *                         (tracs_tree_write_support); n < 4: no labels, NA.  replicate_trees_path != NULL: each replicate's Newick
 *                         line (no labels) is appended to it, in replicate order (n >= 4).  Bit-reproducible for a given (handle,
 *                         replicates, seed).  transfer != 0 (`--bootstrap-support transfer`; needs replicates): the
 *                         same main tree, replicates and replicate_trees_path bytes, with the transfer support beside the split
 *                         count: after the main tree tracs_transfer_init, per replicate (after tracs_tree_support) its program and
 *                         transfer_phi_kernel, after the last one tracs_transfer_emit.  The Newick labels are the transfer supports
 *                         and the edge rows carry support,transfer (tracs_tree_write_transfer).
 *                         changes != 0 (`--tree-changes / --tree-sites`; either kind): tracs_fitch_count on the main
 *                         tree.  changes_path != NULL (or filter) and more than max_entries changes in all: refused with a message
 *                         that states it, before any file is touched.  create != 0: the files are then created (the edge file with
 *                         the header parent,child,length,changes,MSA file, the change file with
 *                         parent,child,contig,position,alleleParent,alleleChild,MSA file, the site file with
 *                         contig,position,changes,minimum,MSA file); 0: they are appended to (a second --msa file).  The edge rows
 *                         gain a changes field (tracs_tree_write_changes); the change rows -- sites ascending, walk order within a
 *                         site, nodes named as in the edge rows, alleles A/C/G/T, contig / position as tracs_distance_pair_sites
 *                         writes them (contig_names, contig_lengths, n_contigs) -- come from tracs_fitch_fill in batches of sites:
 *                         two buffers (device, pinned host) of at most 256 MiB (TRACS_FITCH_BATCH: entries per batch, diagnostic),
 *                         rows formatted on n_threads host threads (<= 0: up to 16); the site rows list the sites with a change.
 *                         filter != 0 (`--tree-filter`; needs changes): the branch filter between the count and the
 *                         files: tracs_fitch_edge_sites, then tracs_filter_recomb_lists on the edges' lists (max_entries bounds
 *                         them whether or not changes_path is given: they hold an entry per change).  The edge file's header is
 *                         parent,child,length,changes,filtered,MSA file (filtered: the changes kept on the edge;
 *                         tracs_tree_write_filtered), the change file's parent,child,contig,position,alleleParent,alleleChild,
 *                         dropped,MSA file (dropped: 0 / 1, from tracs_fitch_mark_dropped on every batch); the site file is
 *                         unchanged.  filtered_path != NULL: one Newick line with the topology and labels of `path` and the kept
 *                         changes as branch lengths (tracs_tree_write).
 *                         The result: n_joins: n - 3; rows_written: the edge rows; n_changes: the tree's parsimony length;
 *                         sum_minimum: the sum of `minimum` over the sites with a change; n_kept: the changes kept in all;
 *                         n_edges_dropped: the edges with a dropped change.  What was not asked for is 0.
 *                         kind | TRACS_TREE_BIONJ (kinds 2 and 3; `--tree bionj`): every tree of the request -- the
 *                         main tree, each bootstrap replicate, each rebuild of tracs_distance_tree_iterate -- is the BIONJ tree
 *                         (tracs_bionj_run on a state of tracs_bionj_state_bytes) of the same distances; everything else reads
 *                         the same 2n - 3 edges.  Kind 3 with replicates is refused as kind 1 is; any other kind is refused.  The
 *                         five entry points below and tracs_distance_tree_iterate pass kind through.                             */
#define TRACS_TREE_BIONJ 2             /* bit 1 of tracs_tree_request.kind: the BIONJ tree (tracs_bionj_run) instead of neighbour joining */
typedef struct tracs_tree_request {
    int kind;                          /* bit 0: 0 snp, 1 per-site; bit 1: TRACS_TREE_BIONJ */
    const char *path, *ref, *edges_path;
    uint32_t replicates;               /* 0: no bootstrap */
    uint64_t seed;
    int transfer;                      /* with replicates: the transfer support as well */
    const char *replicate_trees_path;
    int changes;                       /* the Fitch passes: --tree-changes / --tree-sites / --tree-filter */
    const char *changes_path, *sites_path;
    int filter;                        /* with changes: the branch filter */
    const char *filtered_path;
    const char *const *contig_names;
    const uint64_t *contig_lengths;
    size_t n_contigs;
    uint64_t max_entries;
    int n_threads, create;
} tracs_tree_request;
typedef struct tracs_tree_result {
    uint64_t n_joins, rows_written, n_changes, sum_minimum, n_kept, n_edges_dropped;
} tracs_tree_result;
int tracs_distance_tree_run(tracs_distance *h, const tracs_tree_request *req, tracs_tree_result *res);
/*   tracs_distance_tree_iterate  `--tree-filter --tree-iterate K` (not in the reference): the branch filter iterated into
 *                         the topology.  it == NULL: tracs_distance_tree_run, byte for byte.  Else the request needs filter and takes no
 *                         replicates, and 1 <= max_iterations <= 100 (TRACS_E_ARG otherwise).  A is the handle's packed alignment after
 *                         every site and sample rule, n samples, L sites.  NJ(X): the tree of tracs_nj_* from alignment X (kind 0 or
 *                         1, the same operation order and tie rule).  V(T): the dropped (edge e, site s) of the branch filter: Fitch's
 *                         two passes of A on T, then the window test per edge.  below(T, e): the samples in the subtree of e's child,
 *                         the side away from T's top node (n = 2: {1}).
 *                             T_0 = NJ(A).  For k = 1 .. K:
 *                                 M_k = A with the cell (i, s) set to N (mask 15 in the four allele planes, and the N plane) for every
 *                                       (e, s) in V(T_{k-1}) and every i in below(T_{k-1}, e); always from A, never from M_{k-1}
 *                                 T_k = NJ(M_k)
 *                                 T_k has the set of non-trivial splits of some T_j, j < k (tracs_tree_support's comparison): stop;
 *                                       same_as = the smallest such j (j = k - 1: converged; smaller: a cycle)
 *                                 k = K without a repeat: stop at the limit (same_as = -1)
 *                         n < 4 has no non-trivial split: T_1 repeats T_0 and the run ends at k = 1; on two samples the final length is
 *                         the pair's filtered distance.  The final tree is the last T_k: it decides `path`, with lengths as NJ(M_k)
 *                         computes them; edges_path, changes_path, sites_path and filtered_path are what the filter request writes,
 *                         for (A, T_final): Fitch of the ORIGINAL alignment on the final tree, and its verdicts.  Nothing is written
 *                         before the loop ends; max_entries is checked against every iteration's change count.  Kind 1 with a pair
 *                         compared over 0 sites after masking is refused by name, and the message names the iteration.  The masked
 *                         cells of tree k are the cells that are not N in A and are N in M_{k+1} (a set, so deterministic).
 *                         M_k lives in one tracs_alignment_clone of A, restored from A between iterations.
 *                         iterations_path != NULL: one row per tree k = 0 .. final is appended (create != 0: after the header
 *                         iteration,changes,kept,dropped,branches with a drop,masked cells,shared splits,same as,MSA file): the counts
 *                         of V(T_k); masked cells (NA on the final row); shared splits: the non-trivial splits of T_k that T_{k-1}
 *                         has (NA for k = 0); same as: same_as on the final row of a run that stopped on a repeat, NA elsewhere.
 *                         res: the result of the filter request for (A, T_final).  ires: iterations: the final k; same_as;
 *                         masked_cells_last: the masked cells of tree final - 1 (the N cells M_final adds to A); mask_work_max: the
 *                         largest W of tracs_alignment_mask_subtrees over the iterations.                                            */
typedef struct tracs_tree_iterate {
    uint32_t max_iterations;
    const char *iterations_path;
} tracs_tree_iterate;
typedef struct tracs_tree_iterate_result {
    uint32_t iterations;
    int32_t same_as;
    uint64_t masked_cells_last, mask_work_max;
} tracs_tree_iterate_result;
int tracs_distance_tree_iterate(tracs_distance *h, const tracs_tree_request *req, const tracs_tree_iterate *it, tracs_tree_result *res,
                                tracs_tree_iterate_result *ires);
/*   tracs_distance_tree   the request {kind, path, ref, edges_path}: the main tree alone                                         */
int tracs_distance_tree(tracs_distance *h, int kind, const char *path, const char *ref, const char *edges_path, uint64_t *n_joins,
                        uint64_t *rows_written);
/*   tracs_distance_tree_changes  that request with changes = 1 and changes_path .. create                                        */
int tracs_distance_tree_changes(tracs_distance *h, int kind, const char *path, const char *ref, const char *edges_path, const char *changes_path,
                                const char *sites_path, const char *const *contig_names, const uint64_t *contig_lengths, size_t n_contigs,
                                uint64_t max_entries, int n_threads, int create, uint64_t *n_joins, uint64_t *rows_written, uint64_t *n_changes,
                                uint64_t *sum_minimum);
/*   tracs_distance_tree_filter  the request of tracs_distance_tree_changes with filter = 1 and filtered_path                     */
int tracs_distance_tree_filter(tracs_distance *h, int kind, const char *path, const char *ref, const char *edges_path, const char *changes_path,
                               const char *sites_path, const char *filtered_path, const char *const *contig_names, const uint64_t *contig_lengths,
                               size_t n_contigs, uint64_t max_entries, int n_threads, int create, uint64_t *n_joins, uint64_t *rows_written,
                               uint64_t *n_changes, uint64_t *sum_minimum, uint64_t *n_kept, uint64_t *n_edges_dropped);
/*   tracs_distance_tree_bootstrap  the request of tracs_distance_tree with replicates (here at least 1), seed, replicate_trees_path */
int tracs_distance_tree_bootstrap(tracs_distance *h, int kind, const char *path, const char *ref, const char *edges_path, uint32_t replicates,
                                  uint64_t seed, const char *replicate_trees_path, uint64_t *n_joins, uint64_t *rows_written);
/*   tracs_distance_tree_bootstrap_transfer  the request of tracs_distance_tree_bootstrap with transfer = 1                       */
int tracs_distance_tree_bootstrap_transfer(tracs_distance *h, int kind, const char *path, const char *ref, const char *edges_path,
                                           uint32_t replicates, uint64_t seed, const char *replicate_trees_path, uint64_t *n_joins,
                                           uint64_t *rows_written);
/*   tracs_distance_histogram `--histogram` (not in the reference): tracs_distance_run's panel loop without rows.  The
 *                         pairs it would write (d <= dist) are counted by SNP distance and class (tracs_hist_*; group: HOST int32[n]
 *                         in the order of tracs_distance_name, label < 0: ungrouped; NULL: every pair ungrouped) in min(L, dist) + 1
 *                         bins; filter != 0: a second histogram takes their filtered distances (tracs_filter_recomb_pairs).  Appends
 *                         "snp,<d>,<within>,<between>,<ungrouped>,<ref>" per non-empty bin, ascending, then the same with "filter".
 *                         n_eligible: the pairs counted (the rows tracs_distance_run would write without metadata).              */
int tracs_distance_histogram(tracs_distance *h, int dist, int filter, const int32_t *group, const char *path, const char *ref,
                             uint64_t *n_eligible, uint64_t *rows_written);
/*   tracs_distance_site_census    tracs_alignment_site_census of what the handle compares (the surviving samples, the kept columns),
 *                         everything on the host: counts_host uint32[6 * tracs_distance_len] (may be NULL), differs_host
 *                         ceil(tracs_distance_len / 64) words (may be NULL), *n_differs (may be NULL).
 *   tracs_distance_write_alignment  that alignment as FASTA (tracs_write_fasta_rows: ".gz" by suffix), samples [sample_begin,
 *                         sample_end) under their names, unpacked in batches of samples -- device buffer, pinned host buffer,
 *                         writer --, so memory does not grow with n: two buffers of at most 256 MiB (one row when a row is
 *                         longer) plus the writer's members.  differing_only != 0: only the columns that differ among ALL the
 *                         handle's samples (census, then tracs_alignment_select_sites under the differs bitmap into a temporary
 *                         handle that is freed again; no such column: refused).  *sites_written: columns per record.  The handle
 *                         is left as it was.                                                                                   */
int tracs_distance_site_census(tracs_distance *h, uint32_t *counts_host, uint64_t *differs_host, size_t *n_differs);
int tracs_distance_write_alignment(tracs_distance *h, const char *path, size_t sample_begin, size_t sample_end, int differing_only,
                                   int n_threads, int gzip_level, size_t *sites_written);
/*   tracs_distance_alignment   the packed alignment the handle compares (the surviving samples, the kept columns); owned by the handle.
 *   tracs_distance_pair_sites  `tracs pair-sites` (not in the reference): `path` is created and receives the header
 *                         sampleA,sampleB,contig,position,alleleA,alleleB,dropped and one row per SNP site of every listed pair
 *                         (rows / cols: HOST uint32[n_pairs], indices into tracs_distance_name), pairs in list order, sites
 *                         ascending.  contig / position: the column in the coordinates of the files read (through the kept-columns
 *                         bitmap), relative to its contig (names and lengths in file order; n_contigs = 0: contig "alignment");
 *                         alleles: "XACMGRSVTWYHKDBN"[mask] of rows[t] and cols[t]; dropped: NA, or with filter != 0 the verdict of
 *                         tracs_pair_sites_fill (1: dropped).  All pairs are counted first; a total above max_entries is refused
 *                         with a message that states it, before the file is touched.  The entries then come in batches of pairs:
 *                         two buffers (device, pinned host) of at most 256 MiB, or of one pair's entries when a pair has more
 *                         (TRACS_PAIR_SITES_BATCH: entries per batch, diagnostic); fill, copy and formatting of a batch run one
 *                         after another (nothing overlaps); rows are formatted on n_threads host threads
 *                         (<= 0: up to 16).  *rows_written: the rows.                                                          */
tracs_alignment *tracs_distance_alignment(tracs_distance *h);
int tracs_distance_pair_sites(tracs_distance *h, const uint32_t *rows, const uint32_t *cols, size_t n_pairs, int filter, uint64_t max_entries,
                              const char *path, const char *const *contig_names, const uint64_t *contig_lengths, size_t n_contigs,
                              int n_threads, uint64_t *rows_written);
void tracs_distance_free(tracs_distance *h);

/* Rows of `tracs distance`'s CSV appended to path (tracs/distance.py:206-258; the caller writes the header, :157):
 *   names[rows[t]],names[cols[t]],str(delta),str(int(snpd)),str(P),str(E(K)),filtered,str(nn),ref
 * floats print exactly as Python's str(float) / str(numpy.float64).  with_dates = 0: "NA" for delta, P, E(K) (:240-258).
 * filt == NULL: "NA" in the filtered column (:204).  k_max < 0: no -K filter; else rows with k_max >= E(K) only (:222). */
int tracs_write_distance_rows(const char *path, const char *const *names, const uint64_t *rows, const uint64_t *cols,
                              const uint64_t *snpd, const uint64_t *filt, const uint64_t *ncomp, const double *delta,
                              const double *p_direct, const double *e_k, size_t n, int with_dates, double k_max,
                              const char *ref, uint64_t *rows_written);

/* `tracs cluster` input (tracs/cluster.py:100-116): distance CSV -> node names in first-appearance order (sampleA before
 * sampleB; ids continue after the n_seed names given, like the reference's function-level table) and the edges whose
 * field `column` (3 snp, 6 filter, 4 direct, 5 expectedK, :90-97) is <= threshold.  The header line is skipped; a field
 * that float() would refuse is an error carrying Python's message.                                                    */
typedef struct tracs_edge_list tracs_edge_list;
int tracs_read_distance_edges(const char *path, int column, double threshold, const char *const *seed_names,
                              size_t n_seed, tracs_edge_list **out);
size_t tracs_edges_count(const tracs_edge_list *e);
uint64_t tracs_edges_rows(const tracs_edge_list *e);          /* data lines read */
size_t tracs_edges_n_names(const tracs_edge_list *e);
const char *tracs_edges_name(const tracs_edge_list *e, size_t i);
const int32_t *tracs_edges_i(const tracs_edge_list *e);
const int32_t *tracs_edges_j(const tracs_edge_list *e);
void tracs_edges_free(tracs_edge_list *e);

/* write_alignment of tracs/combine.py:220-239: one single-record FASTA per sample -> "<ref>_combined.fasta.gz" with
 * records ">sample\nSEQUENCE\n" in input order.  Samples are compressed in parallel as separate gzip members
 * (n_threads <= 0: all cores; gzip_level < 0: 6).  frac_n[s] = count('N')/len, lengths[s] = len (the ncov dict);
 * a file with more than one record is an error ("... contains more than one sequence").                         */
int tracs_combine_fasta(const char *out_path, const char *const *sample_names, const char *const *fasta_paths,
                        size_t n, int n_threads, int gzip_level, double *frac_n, uint64_t *lengths);

/* Rows of text as FASTA: ">" names[k] "\n" the L bytes at ascii_host + k * stride "\n", k < count, one line per record.  Plain
 * text unless path ends in ".gz": then one gzip member per record, compressed in parallel (n_threads <= 0: all cores; gzip_level
 * < 0: 6) and written in order, as tracs_combine_fasta does.  append != 0 extends the file (a multi-member gzip stays one stream),
 * else it is truncated; count = 0 leaves an empty (or unchanged) file.  Host only.                                            */
int tracs_write_fasta_rows(const char *path, const char *const *names, const uint8_t *ascii_host, size_t stride, size_t count,
                           size_t L, int append, int n_threads, int gzip_level);

/* ===================================================================================== */
/* (4) MULTI-GPU EXCHANGE -- RCCL over xGMI, one communicator rank per process             */
/* ===================================================================================== */

/* The reference is one process (OpenMP, src/pairsnp.hpp:380-382); SURVEY.md 8e / north_star: the pair space is block-
 * partitioned over the GPUs of one node, every rank holds the packed alignment, no collective during compute, the per-rank
 * distance panels are exchanged at the end.  These entry points are that exchange (csrc/comm.cpp over rccl.h; RCCL is opened
 * when the first communicator is made, so a single-GPU host needs none).  Every call enqueues on `stream` of the CURRENT
 * device (hipSetDevice before tracs_comm_create) and returns; results are valid once the stream has reached them.
 *   tracs_comm_unique_id   rank 0 draws an id (TRACS_COMM_ID_BYTES bytes) and hands it to the other ranks by any host means
 *   tracs_comm_create      collective: every rank of the job calls it with the same id and its own rank
 *   tracs_bcast_planes     the packed planes of `root` (the rank that read the FASTA) -> every rank's handle of the same
 *                          shape; the receiving handles forget every derived form (tracs_alignment_touch)
 *   tracs_allgather_panels in place: every rank lays out `base` alike, rank q's block is the `bytes` bytes at
 *                          base + offsets[q] (offsets: host array of `world` entries); afterwards every rank holds every block.
 *                          Row panels of a row-major pair matrix are such blocks (tracs_amd/partition.py)
 *   tracs_allreduce        dtype 0 int64, 1 float64, 2 uint32, 3 uint8; op 0 sum, 1 max, 2 min; in place
 *   tracs_reduce_scatter   in place: buf holds world blocks of count_per_rank elements; afterwards block `rank` of this rank's buf
 *                          is the reduction of every rank's block `rank`.  The site-sharded form of the path: d and the
 *                          compared-sites counts are sums over sites (pairsnp.hpp:398-403,417-420), so ranks that each hold a slice
 *                          of the sites compute all pairs over their slice and the sums arrive as row panels
 *   tracs_alltoall         send / recv hold `world` blocks of block_bytes bytes: block q of send -> rank q, where it becomes block
 *                          `rank` of recv (ncclAllToAll: every pair of ranks over its own xGMI link)
 *   tracs_tri_pack / _sum  the compact form of the site-sharded exchange (csrc/exchange.hip): the cells (i, j >= max(col_begin,
 *                          i + 1)) of the rows [row_begin, row_end) of a uint32 panel (mat indexed by ABSOLUTE row, leading
 *                          dimension ld) packed in `width` = 2 or 4 bytes per cell at element row_slot[i - row_begin] of `packed` (NULL: statistics only)
 *                          (device array; UINT64_MAX: skip the row), as mat[i][j] or, negate != 0, as base - mat[i][j] (the
 *                          compared-sites counts travel as their deficit below the slice's length); stats[0] = largest value
 *                          packed (atomic max), stats[1] += values that did not fit 16 bits.  _sum: mat[i][j] += add +/- the sum
 *                          over the blocks b != skip_block of recv[b * block_elems + row_slot[i - row_begin] + j - first column]
 *   tracs_send / _recv     `bytes` bytes to / from rank `peer` (variable-length COO payloads to the rank that writes the CSV)
 *   tracs_comm_rank / _world  what RCCL reports for the communicator (ncclCommUserRank / ncclCommCount); tracs_rccl_version:
 *                          ncclGetVersion (0: RCCL not available) */
#define TRACS_COMM_ID_BYTES 128
typedef struct tracs_comm tracs_comm;
int tracs_comm_unique_id(void *id, size_t cap);
int tracs_comm_create(const void *id, int rank, int world, tracs_comm **out);
void tracs_comm_free(tracs_comm *c);
int tracs_comm_rank(const tracs_comm *c);
int tracs_comm_world(const tracs_comm *c);
int tracs_bcast(tracs_comm *c, void *buf, size_t bytes, int root, void *stream);
int tracs_bcast_planes(tracs_comm *c, tracs_alignment *a, int root, void *stream);
int tracs_allgather_panels(tracs_comm *c, void *base, const size_t *offsets, size_t bytes, void *stream);
int tracs_allreduce(tracs_comm *c, void *buf, size_t count, int dtype, int op, void *stream);
int tracs_reduce_scatter(tracs_comm *c, void *buf, size_t count_per_rank, int dtype, int op, void *stream);
int tracs_alltoall(tracs_comm *c, const void *send, void *recv, size_t block_bytes, void *stream);
int tracs_tri_pack(const void *mat, size_t ld, size_t n, size_t row_begin, size_t row_end, size_t col_begin, const uint64_t *row_slot,
                   int width, uint32_t base, int negate, void *packed, uint32_t *stats, void *stream);
int tracs_tri_sum(void *mat, size_t ld, size_t n, size_t row_begin, size_t row_end, size_t col_begin, const uint64_t *row_slot, int width,
                  const void *recv, size_t block_elems, int n_blocks, int skip_block, uint32_t add, int negate, void *stream);
int tracs_rccl_version(void);
int tracs_send(tracs_comm *c, const void *buf, size_t bytes, int peer, void *stream);
int tracs_recv(tracs_comm *c, void *buf, size_t bytes, int peer, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRACS_HIP_H */
