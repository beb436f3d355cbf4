"""ctypes binding of libtracs_hip.so (include/tracs_hip.h).

The HIP library IS the product: there is no CPU fallback.  If the shared library is missing,
does not load, or no GPU is visible, calls raise -- they never route through oracle/.

Every entry point is one row of BINDINGS (declared in include/tracs_hip.h) or DEBUG_BINDINGS (the diagnostics of
tracs_amd/csrc/debug_api.h): name -> (restype, [argtypes]); load() applies the rows.  A new entry point takes one prototype
in its header and one row here, and no test of its own for declaration, export or binding: tests/test_bindings.py compares
every row with its prototype, the library's exported symbols with the rows, and the structs and constants below with the header.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtracs_hip.so")
_lib = None

# TRACS_E_* (include/tracs_hip.h): what an entry point returns instead of 0
E_ARG, E_FASTA, E_RAGGED, E_OPEN, E_HIP, E_NOMEM, E_INTERRUPTED = -1, -2, -4, -5, -6, -7, -8

P = C.POINTER
vp, cs, ci, sz, dbl = C.c_void_p, C.c_char_p, C.c_int, C.c_size_t, C.c_double
i32, i64, u32, u64 = C.c_int32, C.c_int64, C.c_uint32, C.c_uint64
vpp, cpp, ip, i32p, u8p, u32p, u64p, szp, fp, dp = P(vp), P(cs), P(ci), P(i32), P(C.c_uint8), P(u32), P(u64), P(sz), P(C.c_float), P(dbl)


class Rules(C.Structure):
    """tracs_rules (include/tracs_hip.h): shares < 0, min_sites = 0 and max_n_samples = 2^32 - 1 mean no rule"""
    _fields_ = [("keep", C.POINTER(C.c_uint64)), ("keep_len", C.c_size_t), ("max_n_share", C.c_double),
                ("max_sample_n_share", C.c_double), ("min_sites", C.c_uint32), ("max_n_samples", C.c_uint32)]


TREE_BIONJ = 2          # TRACS_TREE_BIONJ (include/tracs_hip.h): bit 1 of TreeRequest.kind


class TreeRequest(C.Structure):
    """tracs_tree_request (include/tracs_hip.h): what `--tree nj` is asked for; zero / NULL means not asked for"""
    _fields_ = [("kind", C.c_int), ("path", C.c_char_p), ("ref", C.c_char_p), ("edges_path", C.c_char_p), ("replicates", C.c_uint32), ("seed", C.c_uint64),
                ("transfer", C.c_int), ("replicate_trees_path", C.c_char_p), ("changes", C.c_int), ("changes_path", C.c_char_p), ("sites_path", C.c_char_p),
                ("filter", C.c_int), ("filtered_path", C.c_char_p), ("contig_names", C.POINTER(C.c_char_p)), ("contig_lengths", C.POINTER(C.c_uint64)),
                ("n_contigs", C.c_size_t), ("max_entries", C.c_uint64), ("n_threads", C.c_int), ("create", C.c_int)]


class TreeResult(C.Structure):
    """tracs_tree_result: the counters of a tree request; what was not asked for is 0"""
    _fields_ = [(name, C.c_uint64) for name in ("n_joins", "rows_written", "n_changes", "sum_minimum", "n_kept", "n_edges_dropped")]


class TreeIterate(C.Structure):
    """tracs_tree_iterate (include/tracs_hip.h): the branch filter iterated into the topology, at most max_iterations times"""
    _fields_ = [("max_iterations", C.c_uint32), ("iterations_path", C.c_char_p)]


class TreeIterateResult(C.Structure):
    """tracs_tree_iterate_result: the final k, the earlier tree it repeats (-1: none), the cells the last mask made N, the largest W"""
    _fields_ = [("iterations", C.c_uint32), ("same_as", C.c_int32), ("masked_cells_last", C.c_uint64), ("mask_work_max", C.c_uint64)]


# include/tracs_hip.h, in its order.  Pointers to device memory, opaque handles, streams and plain host buffers are vp.
BINDINGS = {
    "tracs_last_error": (cs, []),
    "tracs_abi_version": (ci, []),
    "tracs_device_count": (ci, []),
    "tracs_pairsnp": (ci, [cpp, ci, ci, ci, ci, vpp]),
    "tracs_pairsnp_len": (sz, [vp]),
    "tracs_pairsnp_nseq": (sz, [vp]),
    "tracs_pairsnp_seqlen": (sz, [vp]),
    "tracs_pairsnp_rows": (u64p, [vp]),
    "tracs_pairsnp_cols": (u64p, [vp]),
    "tracs_pairsnp_distances": (u64p, [vp]),
    "tracs_pairsnp_filt_distances": (u64p, [vp]),
    "tracs_pairsnp_ncompared": (u64p, [vp]),
    "tracs_pairsnp_name": (cs, [vp, sz]),
    "tracs_pairsnp_free": (None, [vp]),
    "tracs_nearest": (ci, [cpp, ci, ci, ci, ci, ci, vpp]),
    "tracs_pairsnp_sites": (ci, [cpp, ci, ci, ci, ci, u64p, sz, u32, vpp]),
    "tracs_nearest_sites": (ci, [cpp, ci, ci, ci, ci, ci, u64p, sz, u32, vpp]),
    "tracs_trans_dist": (ci, [i32p, dp, sz, dbl, dbl, dbl, dp, dp]),
    "tracs_lprob_k_given_N": (ci, [u64p, u64p, dp, sz, dbl, dbl, dp, sz, dp, dp]),
    "tracs_calculate_posteriors": (ci, [dp, sz, sz, dp, ci, dbl, dp]),
    "tracs_find_dirichlet_priors": (ci, [dp, sz, sz, ci, dbl, ci, dbl, dp, ip]),
    "tracs_connected_components": (ci, [i32p, i32p, sz, sz, i32p, i32p]),
    "tracs_alignment_create": (ci, [sz, sz, vpp]),
    "tracs_alignment_free": (None, [vp]),
    "tracs_alignment_n": (sz, [vp]),
    "tracs_alignment_len": (sz, [vp]),
    "tracs_alignment_bytes": (sz, [vp]),
    "tracs_alignment_planes": (vp, [vp]),
    "tracs_alignment_touch": (ci, [vp]),
    "tracs_alignment_hint_rows": (ci, [vp, szp, ci]),
    "tracs_alignment_pack": (ci, [vp, vp, sz, sz, ci, vp]),
    "tracs_alignment_from_fasta": (ci, [cpp, ci, vpp, vpp, szp, szp]),
    "tracs_free": (None, [vp]),
    "tracs_alignment_site_n_counts": (ci, [vp, vp, vp]),
    "tracs_alignment_select_sites": (ci, [vp, u64p, sz, u32, vpp, u64p, szp, vp]),
    "tracs_alignment_sample_n_counts": (ci, [vp, u64p, sz, vp, vp]),
    "tracs_alignment_select_samples": (ci, [vp, u8p, vpp, vp]),
    "tracs_pairs_min_sites": (ci, [vp, vp, sz, sz, sz, sz, sz, i32, u32, vp]),
    "tracs_alignment_site_census": (ci, [vp, vp, u64p, szp, vp]),
    "tracs_alignment_unpack": (ci, [vp, sz, sz, vp, sz, vp]),
    "tracs_pairsnp_rules": (ci, [cpp, ci, ci, ci, ci, P(Rules), vpp]),
    "tracs_nearest_rules": (ci, [cpp, ci, ci, ci, ci, ci, P(Rules), vpp]),
    "tracs_pairsnp_source_nseq": (sz, [vp]),
    "tracs_pairsnp_source_name": (cs, [vp, sz]),
    "tracs_pairsnp_source_n_count": (u32, [vp, sz]),
    "tracs_pairsnp_source_kept": (ci, [vp, sz]),
    "tracs_pairsnp_rule_sites": (sz, [vp]),
    "tracs_pairsnp_dense": (ci, [vp, sz, sz, sz, vp, vp, sz, vp]),
    "tracs_pairsnp_notify_distances": (None, [vp]),
    "tracs_set_stream_policy": (None, [ci]),
    "tracs_pairsnp_dense_thr": (ci, [vp, sz, sz, sz, vp, vp, sz, i32, vp]),
    "tracs_coo_count": (ci, [vp, sz, sz, sz, sz, sz, i32, vp, vp]),
    "tracs_coo_fill": (ci, [vp, vp, sz, sz, sz, sz, sz, i32, vp, vp, vp, vp, vp, vp]),
    "tracs_coo_fill_f64": (ci, [vp, sz, sz, sz, sz, sz, i32, vp, vp, vp, vp, vp, vp]),
    "tracs_edges_count_f64": (ci, [vp, vp, sz, sz, sz, sz, sz, i32, dbl, vp, vp]),
    "tracs_edges_fill_f64": (ci, [vp, vp, sz, sz, sz, sz, sz, i32, dbl, vp, vp, vp, vp, vp]),
    "tracs_knn_state_bytes": (sz, [sz, ci]),
    "tracs_knn_init": (ci, [vp, sz, ci, vp]),
    "tracs_knn_update": (ci, [vp, vp, sz, sz, sz, sz, sz, i32, ci, ci, vp, vp]),
    "tracs_knn_emit": (ci, [vp, sz, sz, ci, vp, vp, vp, vp, vp, vp]),
    "tracs_msf_state_bytes": (sz, [sz]),
    "tracs_msf_init": (ci, [vp, sz, vp]),
    "tracs_msf_update_coo": (ci, [vp, sz, sz, vp, vp, vp, ci, vp, dbl, vp, vp, vp, vp, vp, u64p, vp]),
    "tracs_msf_emit": (ci, [vp, sz, szp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "tracs_anc_state_bytes": (sz, [sz]),
    "tracs_anc_init": (ci, [vp, sz, vp, vp]),
    "tracs_anc_update_coo": (ci, [vp, sz, sz, vp, vp, vp, ci, vp, dbl, vp, vp, vp, vp, vp, u64p, vp]),
    "tracs_anc_emit": (ci, [vp, sz, szp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "tracs_nj_state_bytes": (sz, [sz]),
    "tracs_nj_init": (ci, [vp, sz, vp]),
    "tracs_nj_load_panel": (ci, [vp, sz, vp, vp, sz, sz, sz, ci, vp]),
    "tracs_nj_load_f64": (ci, [vp, sz, vp, sz, vp]),
    "tracs_nj_run": (ci, [vp, sz, vp]),
    "tracs_nj_emit": (ci, [vp, sz, szp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "tracs_nj_edges": (ci, [sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, szp]),
    "tracs_tree_write": (ci, [cpp, sz, vp, vp, vp, sz, cs, cs, cs]),
    "tracs_bionj_state_bytes": (sz, [sz]),
    "tracs_bionj_run": (ci, [vp, sz, vp]),
    "tracs_tree_write_changes": (ci, [cpp, sz, vp, vp, vp, sz, vp, cs, cs, cs]),
    "tracs_tree_write_filtered": (ci, [cpp, sz, vp, vp, vp, sz, vp, vp, cs, cs, cs]),
    "tracs_bootstrap_weights": (ci, [sz, u64, u64, vp, vp]),
    "tracs_alignment_gather_sites": (ci, [vp, vp, vpp, szp, vp]),
    "tracs_tree_support": (ci, [sz, vp, vp, sz, vp, vp, sz, vp]),
    "tracs_tree_write_support": (ci, [cpp, sz, vp, vp, vp, sz, vp, u32, cs, cs, cs]),
    "tracs_tree_transfer_program": (ci, [sz, vp, vp, sz, vp, szp]),
    "tracs_transfer_state_bytes": (sz, [sz]),
    "tracs_transfer_init": (ci, [vp, sz, vp, vp, sz, vp]),
    "tracs_transfer_add": (ci, [vp, sz, vp, vp, sz, vp, vp]),
    "tracs_transfer_emit": (ci, [vp, sz, vp, vp]),
    "tracs_tree_transfer": (ci, [sz, vp, vp, sz, vp, vp, sz, vp]),
    "tracs_tree_write_transfer": (ci, [cpp, sz, vp, vp, vp, sz, vp, vp, vp, u32, cs, cs, cs]),
    "tracs_hist_state_bytes": (sz, [sz]),
    "tracs_hist_init": (ci, [vp, sz, vp]),
    "tracs_hist_update": (ci, [vp, sz, sz, sz, sz, sz, i32, vp, vp, sz, vp]),
    "tracs_hist_update_coo": (ci, [vp, vp, vp, sz, vp, vp, sz, vp]),
    "tracs_hist_emit": (ci, [vp, sz, szp, vp, vp, vp, vp, vp]),
    "tracs_filter_recomb_device": (ci, [vp, vp, vp, sz, vp, vp, vp, vp, vp]),
    "tracs_filter_recomb_pairs": (ci, [vp, vp, vp, vp, sz, vp, vp]),
    "tracs_pair_sites_count": (ci, [vp, vp, vp, sz, vp, vp, u64p, vp]),
    "tracs_pair_sites_fill": (ci, [vp, vp, vp, sz, vp, i64, vp, vp, sz, ci, vp]),
    "tracs_fitch_count": (ci, [vp, vp, vp, sz, vp, vp, vp, vp, u64p, vp]),
    "tracs_fitch_fill": (ci, [vp, vp, vp, sz, sz, sz, vp, i64, vp, vp, vp, sz, vp]),
    "tracs_fitch_edge_sites": (ci, [vp, vp, vp, sz, vp, vp, vp, sz, vp]),
    "tracs_filter_recomb_lists": (ci, [vp, vp, vp, sz, sz, vp, vp, vp]),
    "tracs_fitch_mark_dropped": (ci, [vp, vp, vp, sz, sz, vp, vp, vp, vp]),
    "tracs_alignment_clone": (ci, [vp, vpp, vp]),
    "tracs_alignment_restore": (ci, [vp, vp, vp]),
    "tracs_alignment_mask_subtrees": (ci, [vp, vp, vp, sz, vp, vp, vp, sz, u64p, vp]),
    "tracs_trans_dist_device": (ci, [vp, vp, sz, dbl, dbl, dbl, ci, vp, vp, vp]),
    "tracs_trans_dist_dense": (ci, [vp, sz, sz, sz, sz, sz, i32, vp, dbl, dbl, dbl, ci, vp, vp, vp]),
    "tracs_trans_dist_dense2": (ci, [vp, sz, sz, szp, ci, sz, i32, vp, dbl, dbl, dbl, ci, vp, vp, vp]),
    "tracs_trans_table_dense": (ci, [vp, sz, sz, sz, sz, sz, i32, vp, dbl, dbl, dbl, ci, ci, u32, u32, vp, vp, vp, vp]),
    "tracs_trans_table_gather": (ci, [vp, sz, sz, sz, sz, sz, i32, vp, u32, u32, vp, vp, ci, vp, vp, vp, vp]),
    "tracs_trans_keys_words": (sz, []),
    "tracs_trans_keys_mark": (ci, [vp, sz, sz, szp, ci, sz, i32, vp, vp, vp]),
    "tracs_trans_keys_merge": (ci, [vp, vp, ci, vp]),
    "tracs_trans_keys_info": (ci, [vp, u64p, vp]),
    "tracs_trans_keys_evaluate": (ci, [vp, u64p, ci, ci, dbl, dbl, dbl, vp, sz, vp]),
    "tracs_trans_keys_gather": (ci, [vp, sz, sz, szp, ci, sz, i32, vp, vp, u64p, vp, ci, sz, ci, vp, vp, vp]),
    "tracs_calculate_posteriors_device": (ci, [vp, sz, sz, dp, ci, dbl, vp, vp]),
    "tracs_posterior_codes_device": (ci, [vp, sz, dp, ci, dbl, vp, vp]),
    "tracs_find_dirichlet_priors_device": (ci, [vp, sz, sz, ci, dbl, ci, dbl, dp, ip, vp]),
    "tracs_debug_digamma": (ci, [dp, sz, dp]),
    "tracs_debug_poison_scratch": (None, [ci]),
    "tracs_debug_scratch_hits": (sz, [u64p, sz]),
    "tracs_posterior_codes_cov_device": (ci, [vp, sz, dp, ci, dbl, u32, dbl, dbl, vp, vp]),
    "tracs_coverage_profile_device": (ci, [vp, sz, vp, sz, vp, vp, vp]),
    "tracs_consensus_codes_device": (ci, [vp, sz, u32, vp, vp]),
    "tracs_coverage_profile_device32": (ci, [vp, sz, vp, sz, vp, vp, vp]),
    "tracs_posterior_codes_cov_device32": (ci, [vp, sz, dp, ci, dbl, u32, dbl, dbl, vp, vp]),
    "tracs_consensus_codes_device32": (ci, [vp, sz, u32, vp, vp]),
    "tracs_codes_to_iupac_device": (ci, [vp, sz, vp, vp]),
    "tracs_alignment_pack_codes": (ci, [vp, vp, sz, vp]),
    "tracs_alignment_pack_codes_batch": (ci, [vp, vp, sz, sz, sz, vp]),
    "tracs_connected_components_device": (ci, [vp, vp, sz, sz, vp, i32p, vp]),
    "tracs_pileup_counts": (ci, [cs, cpp, u64p, sz, ci, dp, u64p]),
    "tracs_write_posterior_csv": (ci, [cs, dp, sz, sz, ci]),
    "tracs_warm_up": (None, []),
    "tracs_distance_open": (ci, [cpp, ci, vpp]),
    "tracs_distance_open_sites": (ci, [cpp, ci, u64p, sz, u32, vpp]),
    "tracs_distance_open_rules": (ci, [cpp, ci, P(Rules), vpp]),
    "tracs_distance_source_nseq": (sz, [vp]),
    "tracs_distance_source_name": (cs, [vp, sz]),
    "tracs_distance_source_n_count": (u32, [vp, sz]),
    "tracs_distance_source_kept": (ci, [vp, sz]),
    "tracs_distance_rule_sites": (sz, [vp]),
    "tracs_distance_source_len": (sz, [vp]),
    "tracs_distance_len": (sz, [vp]),
    "tracs_distance_kept_sites": (ci, [vp, u64p]),
    "tracs_distance_nseq": (sz, [vp]),
    "tracs_distance_name": (cs, [vp, sz]),
    "tracs_distance_run": (ci, [vp, ci, i32p, dbl, dbl, dbl, dbl, cs, cs, ci, u64p, u64p]),
    "tracs_distance_forest": (ci, [vp, ci, i32p, dbl, dbl, dbl, dbl, ci, ci, cs, cs, u64p, u64p]),
    "tracs_distance_ancestors": (ci, [vp, ci, i32p, dbl, dbl, dbl, dbl, ci, ci, cs, cs, cs, cpp, u64p, u64p]),
    "tracs_distance_tree_run": (ci, [vp, P(TreeRequest), P(TreeResult)]),
    "tracs_distance_tree_iterate": (ci, [vp, P(TreeRequest), P(TreeIterate), P(TreeResult), P(TreeIterateResult)]),
    "tracs_distance_tree": (ci, [vp, ci, cs, cs, cs, u64p, u64p]),
    "tracs_distance_tree_changes": (ci, [vp, ci, cs, cs, cs, cs, cs, cpp, u64p, sz, u64, ci, ci, u64p, u64p, u64p, u64p]),
    "tracs_distance_tree_filter": (ci, [vp, ci, cs, cs, cs, cs, cs, cs, cpp, u64p, sz, u64, ci, ci, u64p, u64p, u64p, u64p, u64p, u64p]),
    "tracs_distance_tree_bootstrap": (ci, [vp, ci, cs, cs, cs, u32, u64, cs, u64p, u64p]),
    "tracs_distance_tree_bootstrap_transfer": (ci, [vp, ci, cs, cs, cs, u32, u64, cs, u64p, u64p]),
    "tracs_distance_histogram": (ci, [vp, ci, ci, i32p, cs, cs, u64p, u64p]),
    "tracs_distance_site_census": (ci, [vp, vp, u64p, szp]),
    "tracs_distance_write_alignment": (ci, [vp, cs, sz, sz, ci, ci, ci, szp]),
    "tracs_distance_alignment": (vp, [vp]),
    "tracs_distance_pair_sites": (ci, [vp, u32p, u32p, sz, ci, u64, cs, cpp, u64p, sz, ci, u64p]),
    "tracs_distance_free": (None, [vp]),
    "tracs_write_distance_rows": (ci, [cs, cpp, u64p, u64p, u64p, u64p, u64p, dp, dp, dp, sz, ci, dbl, cs, u64p]),
    "tracs_read_distance_edges": (ci, [cs, ci, dbl, cpp, sz, vpp]),
    "tracs_edges_count": (sz, [vp]),
    "tracs_edges_rows": (u64, [vp]),
    "tracs_edges_n_names": (sz, [vp]),
    "tracs_edges_name": (cs, [vp, sz]),
    "tracs_edges_i": (i32p, [vp]),
    "tracs_edges_j": (i32p, [vp]),
    "tracs_edges_free": (None, [vp]),
    "tracs_combine_fasta": (ci, [cs, cpp, cpp, sz, ci, ci, dp, u64p]),
    "tracs_write_fasta_rows": (ci, [cs, cpp, vp, sz, sz, sz, ci, ci, ci]),
    "tracs_comm_unique_id": (ci, [vp, sz]),
    "tracs_comm_create": (ci, [vp, ci, ci, vpp]),
    "tracs_comm_free": (None, [vp]),
    "tracs_comm_rank": (ci, [vp]),
    "tracs_comm_world": (ci, [vp]),
    "tracs_bcast": (ci, [vp, vp, sz, ci, vp]),
    "tracs_bcast_planes": (ci, [vp, vp, ci, vp]),
    "tracs_allgather_panels": (ci, [vp, vp, szp, sz, vp]),
    "tracs_allreduce": (ci, [vp, vp, sz, ci, ci, vp]),
    "tracs_reduce_scatter": (ci, [vp, vp, sz, ci, ci, vp]),
    "tracs_alltoall": (ci, [vp, vp, vp, sz, vp]),
    "tracs_tri_pack": (ci, [vp, sz, sz, sz, sz, sz, vp, ci, u32, ci, vp, vp, vp]),
    "tracs_tri_sum": (ci, [vp, sz, sz, sz, sz, sz, vp, ci, vp, sz, ci, ci, u32, ci, vp]),
    "tracs_rccl_version": (ci, []),
    "tracs_send": (ci, [vp, vp, sz, ci, vp]),
    "tracs_recv": (ci, [vp, vp, sz, ci, vp]),
}

# tracs_amd/csrc/debug_api.h, in its order: exported and bound, but in no public header
DEBUG_BINDINGS = {
    "tracs_debug_iupac_mask": (ci, [ci]),
    "tracs_debug_tile_variant": (cs, []),
    "tracs_debug_mfma_shape": (cs, []),
    "tracs_debug_alignment_encoding": (ci, [vp]),
    "tracs_debug_alignment_kernel": (ci, [vp]),
    "tracs_debug_alignment_site_classes": (ci, [vp, u64p]),
    "tracs_debug_alignment_nw_gram": (ci, [vp]),
    "tracs_debug_alignment_count_source": (ci, [vp, u64p]),
    "tracs_debug_pair_timing": (None, [ci]),
    "tracs_debug_pair_ms_mean": (ci, [ci, fp]),
    "tracs_debug_last_pair_ms": (ci, [fp]),
    "tracs_debug_force_site_classes": (None, [ci]),
    "tracs_debug_pack_timing": (None, [ci]),
    "tracs_debug_pack_stages": (ci, [cs, sz, fp, ci]),
    "tracs_debug_pack_stage_bytes": (ci, [dp, dp, ci]),
    "tracs_debug_site_select_timing": (ci, [vp, u64p, sz, u32, ci, fp, szp, ip]),
    "tracs_debug_sample_select_timing": (ci, [vp, u64p, sz, u8p, ci, fp, szp]),
    "tracs_debug_lists": (sz, [vp, ci, vp, sz]),
    "tracs_debug_filter_index": (ci, [vp, dp]),
    "tracs_debug_last_trans_dist_keys": (u64, []),
    "tracs_debug_trans_routes": (ci, [dp]),
    "tracs_debug_hist_routes": (ci, [vp, dp]),
    "tracs_debug_bootstrap_replicate": (ci, [vp, sz, u64p, u64, u64, dp, vpp, szp]),
    "tracs_debug_transfer_init": (ci, [vp, sz, vp, vp, sz, dp]),
    "tracs_debug_differs_table": (ci, [vp, sz]),
    "tracs_debug_tree_edges_header": (ci, [ci, ci, ci, ci, cs, sz]),
    "tracs_debug_alloc_stats": (None, [u64p]),
    "tracs_debug_fail_alloc": (None, [C.c_long]),
    "tracs_debug_format_floats": (C.c_long, [dp, sz, cs, sz]),
    "tracs_debug_read_fasta": (ci, [cs, szp, szp, u64p]),
}

# every symbol include/tracs_hip.h declares (tests/test_cabi.py checks the .so exports them all)
SYMBOLS = list(BINDINGS)


class TracsError(RuntimeError):
    pass


def _share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64.so (soname libamdhip64.so.7, but torch links it as
    `libamdhip64.so`).  If our library pulled in /opt/rocm's copy first, a later `import torch` would load a
    SECOND HIP runtime into the process and one of the two would see no device.  So when torch is installed,
    its copy is loaded first (no torch import needed); our DT_NEEDED libamdhip64.so.7 then resolves to it."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def load():
    """Load the library (building nothing: run `python -m tracs_amd.build` or __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    _share_hip_runtime_with_torch()
    if not os.path.exists(LIB_PATH):
        raise TracsError("libtracs_hip.so is missing (%s): build it with `python -m tracs_amd.build`; "
                         "there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**BINDINGS, **DEBUG_BINDINGS}.items():
        f = getattr(L, name)                    # a name the library does not export: ctypes' AttributeError, as it is
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc):
    """Raise RuntimeError with the library's message (the reference raises RuntimeError with the
    same strings: src/pairsnp.hpp:86,96-97,342) on a non-zero return code."""
    if rc == E_INTERRUPTED:                        # Ctrl-C arrived while the library held the call
        raise KeyboardInterrupt("Interrupted by user!")
    if rc != 0:
        msg = load().tracs_last_error()
        raise RuntimeError(msg.decode("utf-8", "replace") if msg else "libtracs_hip error %d" % rc)


def require_gpu():
    L = load()
    if L.tracs_device_count() <= 0:
        raise TracsError("no MI355X/HIP device visible: the TRACS distance path runs on the GPU only "
                         "(there is no CPU fallback)")
    return L
