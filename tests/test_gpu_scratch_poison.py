"""Every family of device entry points once more, on memory the library does not own filled with a known byte.

Scratch slots (csrc/common.h, WS_*) are grow-only and shared by every entry point: a fresh slot reads as zero, a reused one holds what
its last user left, and the states and outputs tracs_amd/device.py allocates with torch.empty hold whatever the caching allocator hands
back.  A read before a write in any of them passes or fails with the order and the sizes of the tests that ran before.  Here that memory
is an input: under the module's fixture every outermost entry-point call first fills every scratch slot of the device with one byte
(device.poison_scratch), a slot that grows inside a call starts as that byte, and torch.empty hands out tensors filled with it --

    0x00  shows a missing "set to all ones / KEY_NONE / +inf",
    0xFF  a missing "set to 0", a sticky error flag, NaN in f64 scratch

-- and the project's own exact comparisons run again, unchanged: the test functions below are the ones of the other GPU modules, imported
with their parametrisation (the small cases of every family).  Where those modules start a child process per case -- switches read once per process
-- the child switches poison on for itself (tests/scratch_poison.py) and reports which slots it was handed.  The last test of the module
requires that every scratch slot was handed out under poison, here or in a child, and that the children did run poisoned.  DESIGN.md 3.24 has the audit
of the slots and the states that this module confirms."""
import json
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import scratch_poison  # noqa: E402

pytestmark = pytest.mark.gpu

# ---- the comparisons that run again (and the module-level fixtures they ask for) --------------------------------------------------------
# the dense pair call: consensus and general encodings, matrix-core and VALU kernels, one launch and the thresholded two passes, row
# panels and column starts, with and without ncomp, the COO forms behind it (40 seeded geometries); site classes on and off, every class
# at once, no dense site, the count pass in place and re-packed, the minority lists and their fix-up, nw_gram and nw_rows
from test_gpu_random import test_dense_entry_points_random_geometry  # noqa: E402,F401
from test_gpu_site_classes import (test_dense_alignment_stays_whole, test_every_class_at_once,  # noqa: E402,F401
                                   test_general_alignment_without_dense_sites, test_no_variable_site, test_repack_redecides,
                                   test_row_hint_builds_lists_for_those_rows_only, test_single_variable_site_and_ragged_classes,
                                   test_site_classes_fuzz, test_site_classes_match_oracle)
from test_gpu_nw_gram import test_forced_on_ordinary_alignments  # noqa: E402,F401
# N co-occurrences from lists: the lists themselves dumped and decoded, the rows' slots and bitmaps (forced either way and by the rule),
# row panels, lists that run into overflow lines.  Their switches are read once per process, so each case is a child process: the
# children enter poison themselves (tests/scratch_poison.py, asked to by the fixture through the environment) and report their slots
from test_gpu_lists import test_lists_against_numpy  # noqa: E402,F401
from test_gpu_row_slots import (test_both_sources_agree, test_row_panels, test_rule_chooses_bitmaps_at_3_percent,  # noqa: E402,F401
                                test_slot_and_line_boundaries)
from test_gpu_site_classes import test_long_n_lists  # noqa: E402,F401
# site and sample selection, the pair rule's veto pass
from test_gpu_site_select import test_results_on_the_selected_handle as test_site_select_results  # noqa: E402,F401
from test_gpu_site_select import test_selected_planes_byte_for_byte as test_site_select_planes  # noqa: E402,F401
from test_gpu_site_select import test_site_n_counts  # noqa: E402,F401
from test_gpu_sample_select import test_results_on_the_selected_handle as test_sample_select_results  # noqa: E402,F401
from test_gpu_sample_select import test_selected_planes_byte_for_byte as test_sample_select_planes  # noqa: E402,F401
from test_gpu_sample_select import test_pairs_min_sites_on_a_panel, test_sample_n_counts  # noqa: E402,F401
# site census and unpack
from test_gpu_site_census import (test_after_select_samples_and_select_sites, test_c_entry_point_optional_outputs,  # noqa: E402,F401
                                  test_differs_is_what_changes_a_distance)
from test_gpu_unpack import SHAPES as UNPACK_SHAPES  # noqa: E402
from test_gpu_unpack import make_case as make_unpack_case  # noqa: E402
from test_gpu_unpack import test_round_trip_byte_for_byte, test_text_and_what_stays_untouched  # noqa: E402,F401
# the filter: index and lists, the long-list routes, the plane scan, the position lists
from test_gpu_pairsnp_ref import (test_filter_recomb_device_equals_the_reference,  # noqa: E402,F401
                                  test_filter_recomb_lists_equals_the_reference_on_the_position_lists,
                                  test_filter_recomb_pairs_equals_the_reference_on_every_route)
from test_gpu_filter_hp import test_boundary_pairs_on_every_route, test_table_rows_are_rebuilt_per_alignment  # noqa: E402,F401
# pair sites: count and fill, a pair per lane and a wave per pair, with and without verdicts
from test_gpu_pair_sites import (test_an_index_outside_the_alignment_is_refused, test_sites_and_masks_equal_the_brute_force,  # noqa: E402,F401
                                 test_verdict_counts_equal_the_oracle, test_verdicts_equal_the_definition_bit_for_bit)
# COO and edges, uint32 and f64
from test_gpu_edges_f64 import (cluster_case, test_coo_fill_f64_matches_numpy, test_edges_match_numpy,  # noqa: E402,F401
                                test_edges_of_rank_and_components, test_offsets_cross_the_scan_tile,
                                test_trans_dist_dense_panels_equal_the_whole_matrix)
# transcluster: per pair and dense, hash and grid routes, with and without the (gap, M) tables; the key split and the key table, parts
# played in turn
from test_gpu_transcluster_hp import (test_array_routes_match_high_precision, test_dense_routes_match_high_precision,  # noqa: E402,F401
                                      test_key_split_matches_high_precision, test_key_table_matches_high_precision)
from test_gpu_keysplit import (test_keys_beyond_the_grid_fall_back, test_mark_merge_info_match_the_standin,  # noqa: E402,F401
                               test_split_keys_equal_the_single_call)
from test_gpu_key_table import (test_inputs_reach_the_wave_and_ratio_kernels, test_partitioned_equals_the_single_call,  # noqa: E402,F401
                                test_row_and_column_bounds)
# posteriors and posterior codes, the Dirichlet fit, connected components
from test_gpu_posterior_routes import (dev, tables, test_codes_at_the_route_edges, test_consensus_codes,  # noqa: E402,F401
                                       test_coverage_profile, torch_mod)
from test_gpu_golden import test_connected_components_device, test_posterior_codes_and_device_posteriors  # noqa: E402,F401
from test_gpu_dirichlet_hp import test_degenerate_answers, test_fit_against_the_definition, test_layouts_give_the_same_bits  # noqa: E402,F401
# the running states: kNN, forest, ancestors, histogram -- several panels and batches, the COO forms
from test_gpu_nearest import test_knn_emit_at_scan_seams, test_knn_update_panel_splits  # noqa: E402,F401
from test_gpu_forest import test_msf_eligibility_mask, test_msf_primitives_against_kruskal  # noqa: E402,F401
from test_gpu_ancestors import (test_anc_cross_batch_by_hand, test_anc_eligibility_mask,  # noqa: E402,F401
                                test_anc_primitives_against_the_definition)
from test_gpu_histogram import test_hist_update_panel_splits, test_histogram_wide_range_takes_every_route  # noqa: E402,F401
# NJ and BIONJ: f64 and panel loads, per site; the tree route on a handle: bootstrap replicates, changes, the iterated filter
from test_gpu_nj import (oracle_pairs, test_oracle_distances, test_per_site_distances_and_a_pair_without_sites,  # noqa: E402,F401
                         test_small_n_and_a_state_is_run_once)
from test_gpu_nj import test_panels_in_any_split_and_with_a_wider_leading_dimension as test_nj_panels  # noqa: E402,F401
from test_gpu_nj import test_records_equal_the_definition_bit_for_bit as test_nj_records  # noqa: E402,F401
from test_gpu_bionj import (handle, test_bootstrap_replicates_are_bionj_trees, test_per_site_distances_take_the_method_too,  # noqa: E402,F401
                            test_state_handling, test_the_iterated_filter_ends_on_bionj_trees,
                            test_the_newick_and_the_edge_file_are_the_references, test_tree_changes_count_on_the_bionj_edges)
from test_gpu_bionj import test_panels_in_any_split_and_with_a_wider_leading_dimension as test_bionj_panels  # noqa: E402,F401
from test_gpu_bionj import test_records_equal_the_definition_bit_for_bit as test_bionj_records  # noqa: E402,F401
# bootstrap weights and gather; transfer support on a state and through the tree route (`outbreak`: test_gpu_transfer's)
from test_gpu_bootstrap import (test_distances_on_a_gathered_handle, test_gathered_planes_byte_for_byte,  # noqa: E402,F401
                                test_weights_equal_the_restatement)
from test_gpu_transfer import (outbreak, test_labels_and_rows_are_the_restatement, test_phi_on_random_trees,  # noqa: E402,F401
                               test_the_state_sums_three_replicates)
# Fitch count and fill, the changes regrouped by edge, the branch filter on them, the marks
from test_gpu_fitch import (test_counts_and_entries_equal_the_definition, test_fill_in_two_ranges_and_nothing_beyond_room,  # noqa: E402,F401
                            test_the_default_slab_gives_the_same, test_two_samples_total_is_their_snp_distance)
from test_gpu_branch_filter import (own_cases, test_edge_lists_equal_the_regrouped_reference, test_lists_filter_on_its_own_edges,  # noqa: E402,F401
                                    test_lists_filter_on_the_pinned_boundary, test_marked_entries_carry_the_verdicts)
# mask_subtrees, clone and restore; --tree-iterate; the triangle exchange's pack and sum
from test_gpu_tree_mask import (test_masked_cells_text_and_planes_equal_the_definition,  # noqa: E402,F401
                                test_the_per_pack_caches_are_rebuilt_after_a_mask, test_the_work_is_run_over_in_ranges)
from test_gpu_tree_iterate import test_per_site_distances as test_tree_iterate_per_site  # noqa: E402,F401
from test_gpu_tree_iterate import test_seeded_imports  # noqa: E402,F401
from test_gpu_exchange import test_tri_pack_and_sum_equal_numpy  # noqa: E402,F401


# Scratch slots that one process on one GPU cannot reach, each with the reason the code gives.  At most four: a condition of this
# module, not a measurement -- a slot that is merely not reached wants another case above.
EXEMPT = {
}
MAX_EXEMPT = 4
# the imported tests that start one child process per case
CHILD_TESTS = {"test_lists_against_numpy", "test_both_sources_agree", "test_row_panels", "test_rule_chooses_bitmaps_at_3_percent",
               "test_slot_and_line_boundaries", "test_long_n_lists"}

# what the dense calls of the module's own process ran on (the fixture's wrapper of device.pairsnp_dense keeps the tally)
_seen = {"kernels": set(), "classes": set(), "thresholded": set(), "count source": set(), "second form": set()}
_reports = {}


def _slot_names():
    text = open(os.path.join(ROOT, "tracs_amd", "csrc", "common.h")).read()
    enum = re.search(r"enum WsSlot : int \{(.*?)\};", text, flags=re.S).group(1)
    names = re.findall(r"\bWS_[A-Z0-9_]+", re.sub(r"//[^\n]*", "", enum))
    assert names[-1] == "WS_SLOT_COUNT"
    return names[:-1]


@pytest.fixture(params=UNPACK_SHAPES, ids=["%dx%d" % s for s in UNPACK_SHAPES])
def case(request, hiplib):
    """test_gpu_unpack's alignments, one per test instead of one per module: around a second parametrised fixture of module scope pytest
    regroups the module's tests, and the poison fixture would go down and up (and its hit counters to zero) between that one's cases"""
    yield from make_unpack_case(*request.param, hiplib)


@pytest.fixture(scope="module", autouse=True, params=[0x00, 0xFF], ids=["0x00", "0xFF"])
def poisoned(request, hiplib, tmp_path_factory):
    """scratch poisoned with the byte, torch.empty and torch.empty_like filled with it, the slots' hit counters at zero; child processes
    are told to do the same and where to report"""
    import torch
    from tracs_amd import device
    byte = request.param
    plain_dense = device.pairsnp_dense

    def pairsnp_dense(aln, dist, ncomp=None, *args, **kw):
        out = plain_dense(aln, dist, ncomp, *args, **kw)
        _seen["kernels"].add(aln.kernel)
        _seen["classes"].add(aln.site_classes is not None)
        _seen["thresholded"].add(kw.get("dist_threshold") is not None)
        if aln.count_source is not None:
            _seen["count source"].add("in place" if aln.count_source[1] else "re-packed" if aln.count_source[0] else "none")
            _seen["second form"].add(aln.nw_form)
        return out

    for v in _seen.values():
        v.clear()
    _reports[byte] = str(tmp_path_factory.mktemp("poison") / "children.jsonl")
    undo = scratch_poison.fill_allocations(torch, byte)
    device.pairsnp_dense = pairsnp_dense
    os.environ[scratch_poison.ENV] = "%d:%s" % (byte, _reports[byte])
    try:
        with device.poison_scratch(byte):
            device.scratch_hits()
            yield byte
    finally:
        os.environ.pop(scratch_poison.ENV, None)
        device.pairsnp_dense = plain_dense
        undo()


def test_the_poison_is_there(poisoned, hiplib):
    """the fixture itself: torch.empty and torch.empty_like hand out the byte in every dtype the wrappers ask for, 0-d and empty tensors
    included"""
    import torch
    for dtype in (torch.uint8, torch.int32, torch.int64, torch.float64):
        t = torch.empty((3, 5), dtype=dtype, device="cuda")
        assert t.view(torch.uint8).eq(poisoned).all().item(), dtype
        assert torch.empty_like(t).view(torch.uint8).eq(poisoned).all().item(), dtype
    assert torch.empty((), dtype=torch.int32, device="cuda").reshape(-1).view(torch.uint8).eq(poisoned).all().item()
    assert torch.empty((0,), dtype=torch.float64, device="cuda").numel() == 0


# ---- last in the module ---------------------------------------------------------------------------------------------------------------
def test_every_scratch_slot_was_handed_out_under_poison(request, poisoned):
    """every slot of WS_SLOT_COUNT, by name, in this process or in a poisoned child; the dense call's three kernels, with and without
    site classes, plain and thresholded, the counting pass in place and re-packed, both sources of the second form's terms; and N
    co-occurrences from lists in poisoned children: the lists dumped, the rows as slots and as bitmaps, the long lists"""
    from tracs_amd import device
    # (the gate counts what ran before it: it has to be the last of the module's tests under its byte, whatever pytest regrouped)
    mine = [it for it in request.session.items if it.fspath == request.node.fspath and getattr(it, "callspec", None) is not None
            and it.callspec.params.get("poisoned") == poisoned]
    assert mine and mine[-1] is request.node, "the slot gate is not the last test of the module under 0x%02X" % poisoned
    hits = device.scratch_hits()
    names = _slot_names()
    assert len(hits) == len(names), (len(hits), len(names))
    assert len(EXEMPT) <= MAX_EXEMPT and set(EXEMPT) <= set(names), EXEMPT
    with open(_reports[poisoned]) as fh:
        children = [json.loads(line) for line in fh]
    tags = sorted(c["tag"] for c in children)
    print("poisoned children under 0x%02X: %s" % (poisoned, ", ".join(tags)))
    assert len(children) == len([it for it in mine if it.originalname in CHILD_TESTS]), tags         # every child ran poisoned and said so
    assert all(c["byte"] == poisoned and len(c["hits"]) == len(names) for c in children), children
    assert any(t.startswith("lists:") for t in tags) and any(t.startswith("long_n_lists:") for t in tags), tags
    assert any(t.startswith("row_slots:") and t.endswith("TRACS_ROW_LISTS=1") for t in tags), tags          # the rows' slots ...
    assert any(t.startswith("row_slots:") and t.endswith("TRACS_ROW_LISTS=0") for t in tags), tags          # ... and their bitmaps
    in_children = [sum(c["hits"][k] for c in children) for k in range(len(names))]
    # (the list build's counters, the most N sites of a row among them, live in WS_SL_CNT: every such child built its lists poisoned)
    assert all(c["hits"][names.index("WS_SL_CNT")] >= 1 for c in children if c["tag"].startswith(("row_slots:", "long_n_lists:"))), children
    print("slot hits under 0x%02X (here + in children): %s" %
          (poisoned, ", ".join("%s %d+%d" % (nm, h, c) for nm, h, c in zip(names, hits, in_children))))
    print("dense routes under 0x%02X: %s" % (poisoned, {k: sorted(map(str, v)) for k, v in _seen.items()}))
    missing = [nm for nm, h, c in zip(names, hits, in_children) if h + c == 0 and nm not in EXEMPT]
    assert not missing, "scratch slots never handed out under poison 0x%02X: %s" % (poisoned, ", ".join(missing))
    assert _seen["kernels"] >= {"valu", "mfma", "mfma-general"}, _seen["kernels"]
    assert _seen["classes"] == {False, True} and _seen["thresholded"] == {False, True}, _seen
    assert _seen["count source"] >= {"in place", "re-packed"}, _seen
    assert _seen["second form"] >= {None, "u-pass", "ns-rows"}, _seen
