/*
 * debug_api.h -- the diagnostics entry points of libtracs_hip.so that include/tracs_hip.h does not declare: what tests, bench.py and
 * scripts/ read about the library's routes, lists and stage times.  Exported and bound (tracs_amd/_lib.py) like the public entry
 * points, but no part of the ABI promise: they change with the code they report on.  Every source file that defines one includes
 * this header, so a definition that disagrees with its declaration does not compile; tests/test_bindings.py compares the
 * declarations with the ctypes table.  The contract of each is at its definition.
 */
#ifndef TRACS_DEBUG_API_H
#define TRACS_DEBUG_API_H

#include "../../include/tracs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pairsnp.hip */
int tracs_debug_iupac_mask(int ch);                                               /* the pack's 4-bit allele mask of one byte */
const char *tracs_debug_tile_variant(void);                                       /* the name of the VALU tile variant in use */
const char *tracs_debug_mfma_shape(void);                                         /* the name of the matrix-core tile shape in use */
int tracs_debug_alignment_encoding(const tracs_alignment *a);                     /* 1 consensus, 0 general encoding of the last dense call, -1 undecided */
int tracs_debug_alignment_kernel(const tracs_alignment *a);                       /* the kernel of the last dense call: 0 VALU, 1, 2 matrix core, -1 none */
int tracs_debug_alignment_site_classes(const tracs_alignment *a, uint64_t *out);  /* the classes' state; out[4]: the sites per class */
int tracs_debug_alignment_nw_gram(const tracs_alignment *a);                      /* whether the minority sites' N terms come from the matrix cores */
int tracs_debug_alignment_count_source(const tracs_alignment *a, uint64_t *out);  /* out[8]: what completes the compared-sites counts */
void tracs_debug_pair_timing(int on);                                             /* switch the HIP events around the stages of a dense call */
int tracs_debug_pair_ms_mean(int n_last, float *out);                             /* out[4]: the stages' mean milliseconds over the last calls */
int tracs_debug_last_pair_ms(float *out);                                         /* out[4]: the same for the last call alone */

/* site_classes.hip */
void tracs_debug_force_site_classes(int mode);                                    /* override TRACS_SITE_CLASSES for handles decided from now on */
void tracs_debug_pack_timing(int on);                                             /* switch the HIP events around the once-per-pack stages */
int tracs_debug_pack_stages(char *names, size_t cap, float *ms, int max_stages);  /* names and milliseconds of the last once-per-pack build */
int tracs_debug_pack_stage_bytes(double *rd, double *wr, int max_stages);         /* bytes read and written by those stages */

/* site_select.hip, sample_select.hip */
int tracs_debug_site_select_timing(const tracs_alignment *src, const uint64_t *keep, size_t keep_len, uint32_t max_n_samples, int repeats,
                                   float *ms, size_t *n_kept, int *same);         /* ms[repeats][4]: the stages of one site selection */
int tracs_debug_sample_select_timing(const tracs_alignment *src, const uint64_t *keep, size_t keep_len, const uint8_t *keep_sample, int repeats,
                                     float *ms, size_t *n_kept);                  /* ms[repeats][2]: the N count and the gather of a sample selection */

/* site_lists.hip, filter_lists.hip */
size_t tracs_debug_lists(const tracs_alignment *a, int what, void *out, size_t cap);    /* one array of the site classes' lists, copied to the host */
int tracs_debug_filter_index(const tracs_alignment *a, double *out);              /* out[10]: size and build times of the filter's departure lists */

/* transcluster.hip */
unsigned long long tracs_debug_last_trans_dist_keys(void);                        /* the distinct keys of the last transcluster call */
int tracs_debug_trans_routes(double *out);                                        /* out[8]: the routes of the last key evaluation */

/* histogram.hip */
int tracs_debug_hist_routes(const void *state, double *out);                      /* out[4]: the cells a state's updates counted, by route */

/* bootstrap.hip, transfer.hip */
int tracs_debug_bootstrap_replicate(const tracs_alignment *var, size_t L, const uint64_t *differs, uint64_t seed, uint64_t replicate,
                                    double *seconds, tracs_alignment **out, size_t *n_out);     /* one replicate, seconds[4] by stage */
int tracs_debug_transfer_init(void *state, size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges,
                              double *seconds);                                   /* tracs_transfer_init, seconds[2]: the host's share and the uploads */

/* msa_out.hip, nj.hip */
int tracs_debug_differs_table(uint8_t *out, size_t bytes);                        /* the 2 048-byte table behind the census's differs bit */
int tracs_debug_tree_edges_header(int support, int transfer, int changes, int filtered, char *out, size_t cap);   /* the edge file's header line */

/* capi.hip: the allocation path (alloc_path.h) */
void tracs_debug_alloc_stats(uint64_t *out);                                      /* out[4]: live device blocks and bytes, live pinned blocks, allocations since the last reading */
void tracs_debug_fail_alloc(long nth);                                            /* the nth allocation from now fails as out of memory, once; 0: off */

/* alignio.cpp, capi.hip */
long tracs_debug_format_floats(const double *x, size_t n, char *buf, size_t cap); /* str(float) of n doubles as the row writer prints them */
int tracs_debug_read_fasta(const char *path, size_t *n, size_t *L, uint64_t *hash);     /* records, length and a hash of a FASTA file as parsed */

#ifdef __cplusplus
}
#endif
#endif /* TRACS_DEBUG_API_H */
