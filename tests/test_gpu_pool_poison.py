"""The bit-exact parity assertions again, on poisoned device scratch.

Every answer of the library is meant to be a pure function of its inputs.  A kernel that reads a
slot of device scratch nobody wrote (a missing zero-fill, an unmasked read of a slack or padding
slot, a counter that is not reset) still passes the suite as long as that slot happens to read as
zeros, which fresh hipMalloc blocks usually do and recycled pool blocks often do.  With
RPT_POOL_POISON=<byte> in the environment the pooled allocator (csrc/api.hip, dev_alloc) fills every
block it hands out, the whole block and not only the bytes asked for, so such a read computes garbage
and the existing assertions against the oracle and the numpy restatements see it.

The variable is read once, when the library is loaded, so each case runs a list of EXISTING gpu
tests (by node id: their assertions are reused, not restated) in a fresh child process.  The list
starts with the probe test of this file, which fails in a child whose allocator does not poison.

What the sweep cannot see: LDS, the pinned staging buffer, buffers the caller or torch allocated
(only their library-side shadows are poisoned), and scratch a context keeps across calls after its
first allocation (poisoned once, when it is first allocated).
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = "tests/test_gpu_pool_poison.py::test_pool_probe_sees_the_poison"

# 255: NaN floats and doubles, -1 ids and counts, every flag set.
# 127: huge finite floats and doubles, huge positive ints: what NaN-last ordering or a `< 0` guard hides.
POISON_BYTES = (255, 127)

_P = "tests/test_gpu_parity.py::"
_A = "tests/test_gpu_abi.py::"
_C = "tests/test_gpu_configs.py::"
_M = "tests/test_gpu_knn_metrics.py::"
_MC = "tests/test_gpu_knn_metric_cut.py::"
_LC = "tests/test_gpu_knn_l2_cut.py::"
_TB = "tests/test_gpu_knn_tier_bounds.py::"
_B = "tests/test_gpu_brute_csr.py::"
_G = "tests/test_gpu_knn_graph.py::"
_GM = "tests/test_gpu_knn_graph_metric.py::"
_GC = "tests/test_gpu_knn_graph_csr.py::"
_R = "tests/test_gpu_knn_graph_refine.py::"
_RM = "tests/test_gpu_knn_graph_refine_metric.py::"
_S = "tests/test_gpu_graph_search.py::"
_SC = "tests/test_gpu_graph_search_csr.py::"
_PR = "tests/test_gpu_graph_prepare.py::"
_PC = "tests/test_gpu_graph_prepare_csr.py::"
_OK = "tests/test_gpu_forest_own_keys.py::"

# family -> (unpoisoned seconds of the node list on an MI355X, the child's time limit, node ids).
# The limit is 5 x the unpoisoned time (poison adds two device synchronisations and a fill per
# allocation; machines differ) and at least 120 s.
FAMILIES = {
    "projection": (4.7, 120, [
        _P + "test_project_exact_f64_bit_identical[777-37-33]",
        _P + "test_project_exact_f64_bit_identical[4099-130-13]",
        _P + "test_project_exact_matches_oracle_inner_sd",
        _P + "test_project_mfma_within_tolerance[777-37-33-float64-1e-13]",
        _P + "test_project_mfma_within_tolerance[4099-200-17-float32-1e-05]",
        _P + "test_project_mfma_within_tolerance[1500-128-230-float64-1e-13]",
        _P + "test_project_mfma_within_tolerance[1200-784-50-float32-1e-05]",
        _P + "test_project_mfma_bf16_input[1111-128-52]",
        _P + "test_project_mfma_bf16_input[4097-200-129]",
        _P + "test_project_mfma_bf16_input[257-72-5]",
        _P + "test_project_bf16_both_kernels_agree",
        _P + "test_project_csr_exact",
        _P + "test_project_csr_dense_mfma[64-float64]",
        _P + "test_project_csr_dense_mfma[200-float32]",
        _A + "test_csr_projection_32_per_pass_is_bit_identical[300-float64]",
        _A + "test_csr_projection_32_per_pass_is_bit_identical[1500-float32]",
        _P + "test_split_segments_matches_partition_at_median",
    ]),
    "forest": (4.9, 120, [
        _P + "test_forest_build_exact_identical[257-5-2-128-3]",
        _P + "test_forest_build_exact_identical[20000-32-4-50-None]",
        _P + "test_forest_build_exact_identical[10000-16-2-3000-4]",
        _P + "test_forest_build_exact_identical[9000-8-2-5000-3]",   # leaves above the LDS sort's 4096 points
        _P + "test_forest_build_exact_identical[3-4-2-0-4]",
        _P + "test_forest_build_sparse_with_ties_identical",
        _P + "test_forest_build_all_identical_points",
        _P + "test_forest_build_mfma_mode_is_valid_tree",
        _P + "test_forest_build_f32",
        _A + "test_every_fallback_option_keeps_the_forest_identical",
        _P + "test_heavy_ties_take_the_fallback_paths[1800]",
        _P + "test_heavy_ties_take_the_fallback_paths[3000]",
        _P + "test_deep_trees_down_to_single_points[9000-3]",
        _P + "test_deep_trees_down_to_single_points[2500-1]",
        _P + "test_more_than_4096_bins_per_node",
        _C + "test_bf16_forest_and_knn_small_all_paths",
        "tests/test_golden.py::test_golden_forest_dense_gpu",
        "tests/test_golden.py::test_golden_forest_sparse_gpu",
        "tests/test_golden.py::test_golden_partition_gpu",
    ]),
    "forest_large": (7.9, 120, [
        _A + "test_streaming_on_16bit_codes_is_exact[exact-ties]",
        _A + "test_streaming_on_16bit_codes_is_exact[mfma-heavy]",
        _A + "test_codes_after_the_projection_for_csr_and_bf16_rows",
        _P + "test_mid_size_nodes_on_packed_codes[300001-128-cont-float64-exact]",
        _P + "test_mid_size_nodes_on_packed_codes[300000-32-clump-float32-auto]",
    ]),
    # the streamed and selection paths (the most scratch) against the split of their own keys
    "forest_own_keys": (6.2, 120, [
        _OK + "test_streamed_levels[f32-dups-131080-16]",
        _OK + "test_streamed_levels[bf16-lattice-131080-64]",               # codes from pcode_kernel
        _OK + "test_mid_size_nodes_on_packed_codes[f32-clump-300001-16-32]",   # csub_kernel, nodes handed back
        _OK + "test_streamed_levels[csr_mfma-dups-131080-64]",              # CSR rows in tolerance mode
        _OK + "test_two_stage_pick[f64_mfma-dups]",
        _OK + "test_below_the_streamed_levels[f32-dups-16-4097-1]",          # no_stream
    ]),
    "forest_stream": (5.5, 120, [
        _P + "test_streaming_forest_is_the_reference_fold_over_chunks[4000-12-3-20-33]",
        _P + "test_streaming_forest_is_the_reference_fold_over_chunks[5000-8-2-0-64]",
        _P + "test_streaming_forest_is_the_reference_fold_over_chunks[20000-16-3-50-7000]",
        _P + "test_queries_on_a_streamed_forest",
        _P + "test_streaming_forest_of_svector_rows[37]",
        _P + "test_streaming_forest_of_svector_rows[3000]",
        _M + "test_metric_on_a_streamed_forest",
        _B + "test_recall_hits_streamed_forest",
    ]),
    "knn": (5.7, 120, [
        _P + "test_candidates_identical",
        _P + "test_knn_matches_oracle[10]",
        _P + "test_knn_matches_oracle[50]",
        _P + "test_knn_dedup",
        _P + "test_knn_more_than_candidates",
        _P + "test_knn_wave_and_workgroup_variants_agree_with_oracle[f64]",
        _P + "test_knn_wave_and_workgroup_variants_agree_with_oracle[f32]",
        _P + "test_large_pivot_bins_selection_path[1]",
        _P + "test_knn_f32_prefilter_is_exact[10-ties]",
        _P + "test_knn_f32_prefilter_is_exact[1-dups]",
        _P + "test_knn_cut_between_two_candidates_an_ulp_apart[default]",
        _P + "test_knn_cut_between_two_candidates_an_ulp_apart[wave]",
        _P + "test_knn_cut_between_two_candidates_an_ulp_apart[general]",
        _P + "test_knn_f32_prefilter_uncertified_queries_rerun",
        _P + "test_knn_f32_prefilter_switches_itself_off_on_self_queries",
        _P + "test_knn_f32_prefilter_out_of_range_data",
        _P + "test_knn_general_path_large_k_and_many_ranges",
        _P + "test_knn_many_trees_slots_and_second_traversal[600]",
        _P + "test_knn_nan_query_is_answered_and_hurts_nobody[1-1]",
        _P + "test_knn_nan_query_is_answered_and_hurts_nobody[1-0]",
        _P + "test_knn_nan_query_is_answered_and_hurts_nobody[0-1]",
        _P + "test_knn_nan_query_is_answered_and_hurts_nobody[0-0]",
        _P + "test_knnh_matches_oracle",
        _P + "test_knnh_sparse_matches_oracle",
        _P + "test_knnpq_collapses_equal_distances",
        _A + "test_knn_vote_matches_keep_counts[f64]",
        _LC + "test_cut_inside_a_band_of_permutations[d37-no_pre32]",   # the exact L2 kernel and its list
        _LC + "test_cut_inside_the_copies_of_a_pair[12-general]",
        _LC + "test_tie_at_the_prefilter_cut_ends_on_the_definition",
    ]),
    "knn_tiers": (4.9, 120, [
        _P + "test_knn_int8_tier_is_exact[ties-shape2]",
        _P + "test_knn_int8_tier_is_exact[clip-shape3]",
        _P + "test_knn_tiers_demote_one_at_a_time",
        _P + "test_knn_f32_data",
        _P + "test_knn_f32_data_half_shadow_tier_changes_nothing[ties-shape3]",
        _P + "test_knn_f32_data_half_shadow_tier_changes_nothing[self-shape4]",
        _C + "test_bf16_int8_ranking_tier_changes_nothing[shape1]",
        # the certificates where the shadow misranks: one case per tier (and the wider retry)
        _TB + "test_aligned_half_ulp_cases[f32-wave-last]",
        _TB + "test_aligned_half_ulp_cases[half-wg_retry-middle]",
        _TB + "test_aligned_half_ulp_cases[f32half-shardn-first]",
        _TB + "test_int8_one_outlier_element[shard8-16]",
        _TB + "test_aligned_csr_cases[csr32-last]",
        _TB + "test_aligned_csr_cases[ell-first]",
    ]),
    "knn_shards": (9.4, 120, [
        _P + "test_knn_shard_kernels_are_exact[ties-shape2-f64]",
        _P + "test_knn_shard_kernels_are_exact[self-shape3-f32]",
        _P + "test_knn_shard_kernels_any_tree_count_and_batch_size[33-64]",
        _P + "test_knn_shard_kernels_any_tree_count_and_batch_size[7-130]",
        _P + "test_knn_shard_list_overflow_goes_to_the_exact_kernel",
        _P + "test_knn_merge_shards",
        _P + "test_knn_merge_records_equals_merge",
        _A + "test_merge_beyond_one_launch[5-700]",
        _A + "test_merge_beyond_one_launch[8-1024]",
        _A + "test_sharded_entry_points_one_gpu_equal_the_plain_ones",
        _A + "test_forced_exchange_runs_allgather_and_merge_on_one_rank",
    ]),
    "knn_csr": (5.6, 120, [
        _P + "test_knn_csr",
        _A + "test_csr_knn_fused_equals_general_path_and_oracle[float64]",
        _A + "test_csr_knn_fused_equals_general_path_and_oracle[float32]",
        _A + "test_csr_knn_with_the_reference_metric_is_bit_identical",
        _A + "test_csr_knn_f32_prefilter_is_exact",
        _A + "test_csr_half_table_is_skipped_when_it_cannot_hold_the_rows",
        _A + "test_csr_dataset_borrowed_from_hbm",
    ]),
    "knn_metric": (7.5, 120, [
        _M + "test_metric_parity_grid[f64-48]",
        _M + "test_metric_parity_grid[f32-128]",
        _M + "test_metric_parity_grid[bf16-48]",
        _M + "test_recall_with_cosine",
        _M + "test_metric_sharded_forced_exchange",
        _M + "test_merge_orders_negative_and_nan_distances",
        _MC + "test_cut_under_cancellation[1e+16-f64]",
        _MC + "test_cut_under_cancellation[100000000.0-f32]",
        _MC + "test_cut_on_wide_ties[33-f32]",
        _MC + "test_cut_on_wide_ties[10-bf16]",
        _MC + "test_cut_nub_on_swapped_lanes[f64]",
        _MC + "test_cut_at_the_lds_ceiling[bf16]",
        _MC + "test_cut_shape_grid[33-f64]",
        _MC + "test_cut_shape_grid[257-f32]",
        _MC + "test_cut_shape_grid[768-bf16]",
        _MC + "test_cut_many_ranges[200-f64]",
        _MC + "test_cut_parity_grid_data_certifies",
        _MC + "test_cut_sharded_forced_exchange",
    ]),
    "brute": (5.4, 120, [
        _P + "test_brute_knn",
        _P + "test_recall_with_matches_oracle",
        _M + "test_metric_brute_force[f64]",
        _M + "test_metric_brute_force[bf16]",
        _MC + "test_cut_brute_force[5-f64]",
        _MC + "test_cut_brute_force[513-f32]",
        _MC + "test_cut_brute_force[1025-bf16]",
        _B + "test_brute_csr_true_l2_matches_numpy[float64-3000-30-0.3]",
        _B + "test_brute_csr_true_l2_matches_numpy[float32-3000-30-0.3]",
        _B + "test_brute_csr_planted_ties",
        _B + "test_brute_csr_reference_metric_is_bit_identical",
        _B + "test_brute_csr_tile_independence[3000-30-0.3]",
        _B + "test_brute_csr_agrees_with_forest_knn",
        _B + "test_recall_hits_csr_forest",
        _B + "test_recall_hits_dense_forest_all_metrics[float64]",
        _B + "test_recall_hits_dense_forest_all_metrics[float32]",
        _B + "test_brute_knn_dev_matches_host",
    ]),
    "knn_graph": (10.6, 120, [
        _G + "test_graph_matches_the_definition[f64-24-10]",
        _G + "test_graph_matches_the_definition[f32-200-64]",
        _G + "test_graph_matches_the_definition[bf16-128-1]",
        _G + "test_leaf_sizes_and_padding[3000-100-5-64]",
        _G + "test_leaf_sizes_and_padding[700-1-12-5]",
        _G + "test_leaf_sizes_and_padding[130-10-1-64]",
        _G + "test_empty_data_set",
        _G + "test_depth_zero_is_all_pairs[f64]",
        _G + "test_wide_ties_order_by_id",
        _G + "test_depth_cap_leaves_of_thousands",
        _G + "test_accumulate_folds_forests_in_any_order[bf16-64]",
        _G + "test_imported_forest",
        _G + "test_dev_entry_point_with_torch_tensors[bf16]",
        _GM + "test_graph_matches_the_definition[cosine-f32-33-10]",
        _GM + "test_graph_matches_the_definition[inner-bf16-200-64]",
        _GM + "test_graph_matches_the_definition[cosine-f64-3-1]",
        _GM + "test_depth_zero_large_leaves_and_tiny_inputs[4500-1-10-cosine]",
        _GM + "test_depth_zero_large_leaves_and_tiny_inputs[100-0-64-inner]",
        _GM + "test_small_integer_rows_tie_widely[400-cosine]",
        _GM + "test_orthogonal_rows_give_negative_zero_and_ties_by_id",
        _GM + "test_scaled_copies_tie_exactly[inner]",
        _GM + "test_accumulate_folds_forests_in_any_order[f64-10-cosine]",
        _GC + "test_graph_matches_the_dense_definition[f64-70-0.05-10]",
        _GC + "test_graph_matches_the_dense_definition[f32-200-0.3-64]",
        _GC + "test_awkward_rows[33-f64]",
        _GC + "test_awkward_rows[1-f32]",
        _GC + "test_wide_rows_with_mostly_empty_windows",
        _GC + "test_leaf_sizes_and_padding[3000-100-5-64]",
        _GC + "test_depth_zero_is_all_pairs[f32]",
        _GC + "test_accumulate_folds_tree_shards_in_any_order[f64-10]",
    ]),
    "knn_graph_refine": (10.2, 120, [
        _R + "test_refine_matches_the_definition[f64-24-10-10-1]",
        _R + "test_refine_matches_the_definition[f32-200-64-64-2]",
        _R + "test_refine_matches_the_definition[bf16-128-10-3-3]",
        _R + "test_two_calls_give_the_same_bits",
        _R + "test_short_and_empty_rows",
        _R + "test_tiny_data_sets[2]",
        _R + "test_nan_row_ranks_last_by_id[f64]",
        _R + "test_wide_ties_enter_by_id",
        _R + "test_fixed_point_after_an_even_and_an_odd_number_of_rounds",
        _R + "test_accumulating_the_forest_into_a_refined_graph_changes_nothing[4]",
        _RM + "test_refine_matches_the_definition[cosine-f32-33-10]",
        _RM + "test_refine_matches_the_definition[inner-bf16-200-64]",
        _RM + "test_one_to_three_rounds_with_reverse_0_3_k[cosine-f64-3-2]",
        _RM + "test_one_to_three_rounds_with_reverse_0_3_k[inner-f32-0-3]",
        _RM + "test_two_calls_give_the_same_bits[inner]",
        _RM + "test_short_and_empty_rows[cosine]",
        _RM + "test_zero_row_ranks_last_by_id_under_cosine",
        _RM + "test_wide_ties_enter_by_id[cosine]",
        _RM + "test_both_zeros_in_one_row",
        _RM + "test_metric_zero_gives_the_bits_of_the_old_entry_points[f32]",
        _GC + "test_refine_matches_the_dense_definition[f64-0.05-10-3]",
        _GC + "test_refine_matches_the_dense_definition[f32-0.3-5-1]",
        _GC + "test_refine_to_the_fixed_point_and_twice_the_same_bits",
        _GC + "test_refine_awkward_rows[f64]",
        _GC + "test_refine_tiny_data_sets[2]",
    ]),
    "graph_search": (6.6, 120, [
        _S + "test_search_matches_the_definition[l2-f64-24-10-1]",
        _S + "test_search_matches_the_definition[cosine-f32-200-64-8]",
        _S + "test_search_matches_the_definition[inner-bf16-24-64-8]",
        _S + "test_search_matches_the_definition[l2-bf16-200-10-8]",
        _S + "test_complete_graph_gives_the_brute_force_answer[l2-f64]",
        _S + "test_complete_graph_gives_the_brute_force_answer[cosine-bf16]",
        _S + "test_no_queries_one_point_and_no_seeds",
        _S + "test_seed_with_an_empty_row_and_disconnected_halves",
        _S + "test_chunk_edges[1-f64-l2]",
        _S + "test_chunk_edges[33-f32-cosine]",
        _S + "test_chunk_edges[33-bf16-inner]",
        _S + "test_wide_rows_beyond_the_resident_query",
        _S + "test_two_calls_and_the_dev_entry_point_give_the_same_bits[cosine]",
        _S + "test_seeds_from_a_forest[l2]",
        _SC + "test_search_matches_the_dense_definition[f64-70-0.05-10-1]",
        _SC + "test_search_matches_the_dense_definition[f32-200-0.3-64-8]",
        _SC + "test_search_matches_the_dense_definition[f64-24-0.3-10-8]",
        _SC + "test_piece_and_cap_edges[1-1]",
        _SC + "test_piece_and_cap_edges[1-256]",
        _SC + "test_piece_and_cap_edges[64-64]",
        _SC + "test_piece_and_cap_edges[64-256]",
        _SC + "test_awkward_values[33-f64]",
        _SC + "test_awkward_values[1-f32]",
        _SC + "test_queries_above_any_resident_cap",
        _SC + "test_complete_graph_gives_the_brute_force_answer",
        _SC + "test_no_queries_no_points_one_point_and_no_seeds",
        _SC + "test_seed_with_an_empty_row_and_disconnected_halves",
        _SC + "test_two_calls_and_the_dev_entry_point_give_the_same_bits",
        _SC + "test_seeds_from_a_forest",
    ]),
    "graph_prepare": (12.2, 120, [
        _PR + "test_prepare_matches_the_definition[f64-24-l2-10]",
        _PR + "test_prepare_matches_the_definition[f32-200-cosine-64]",
        _PR + "test_prepare_matches_the_definition[bf16-24-inner-11]",
        _PR + "test_prepare_matches_the_definition[bf16-200-l2-1]",
        _PR + "test_chunk_edges[1-f64-l2]",
        _PR + "test_chunk_edges[33-f32-cosine]",
        _PR + "test_chunk_edges[33-bf16-inner]",
        _PR + "test_wide_rows",
        _PR + "test_hub_empty_rows_and_tiny_sets",
        _PR + "test_inconsistent_distances_row_i_wins",
        _PR + "test_two_calls_and_the_dev_entry_point_give_the_same_bits[inner]",
        _PR + "test_search_on_a_prepared_graph[cosine]",
        _PC + "test_prepare_matches_the_dense_definition[f64-70-0.05-10]",
        _PC + "test_prepare_matches_the_dense_definition[f32-200-0.3-64]",
        _PC + "test_prepare_matches_the_dense_definition[f64-24-0.3-11]",
        _PC + "test_cap_and_length_edges",
        _PC + "test_awkward_values[33-f64]",
        _PC + "test_awkward_values[1-f32]",
        _PC + "test_a_long_row_among_the_neighbours",
        _PC + "test_sixty_four_long_neighbours",
        _PC + "test_hub_empty_rows_and_tiny_sets",
        _PC + "test_inconsistent_distances_row_i_wins",
        _PC + "test_two_calls_and_the_dev_entry_point_give_the_same_bits",
        _PC + "test_search_on_a_prepared_graph",
    ]),
}

# exit statuses of a child that died instead of failing: abort, segmentation fault, time limit
DEAD_STATUSES = (134, 139, 124, 137)
_dead_child = None        # set by the first child that died: no process is started after it


def child_command(nodes):
    return [sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", PROBE] + list(nodes)


@pytest.mark.skipif("RPT_POOL_POISON" not in os.environ,
                    reason="runs in the children of test_parity_under_poison (RPT_POOL_POISON is not set here)")
def test_pool_probe_sees_the_poison():
    import numpy as np
    import rptree_amd as rp
    want = int(os.environ["RPT_POOL_POISON"])
    assert 0 <= want <= 255
    ctx = rp.default_context()
    for cycle in range(2):
        for nbytes in (1000, 3 << 20):       # a 256-byte-granular block and a 2 MB-granular one
            got, poison = ctx.pool_probe(nbytes)
            assert poison == want, (cycle, nbytes, poison)
            got = np.frombuffer(got, dtype=np.uint8)
            assert got.size == nbytes
            assert (got == want).all(), (cycle, nbytes, np.flatnonzero(got != want)[:8])
        # real work between the cycles: its blocks (a 2.5 MB data set among them) go back to the
        # pool with data in them, and the probes of the second cycle are served from recycled blocks
        X = np.random.default_rng(cycle).standard_normal((20000, 16))
        rp.project(X, X[:8].copy(), mode=rp.RPT_PROJ_EXACT, ctx=ctx)
        ctx.sync()


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("byte", POISON_BYTES)
def test_parity_under_poison(byte, family):
    global _dead_child
    if _dead_child is not None:
        pytest.fail("no child is started after a child that died: " + _dead_child)
    _, limit, nodes = FAMILIES[family]
    env = dict(os.environ)
    env["RPT_POOL_POISON"] = str(byte)
    cmd = ["timeout", "-k", "10", str(limit)] + child_command(nodes)
    try:
        pr = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                            timeout=limit + 30)
    except subprocess.TimeoutExpired as e:
        _dead_child = "%s under poison %d did not end within %d s" % (family, byte, limit + 30)
        pytest.fail(_dead_child + "\n" + (e.stdout or b"").decode("utf-8", "replace")[-4000:])
    tail = pr.stdout.decode("utf-8", "replace")[-4000:]
    if pr.returncode < 0 or pr.returncode in DEAD_STATUSES:
        _dead_child = "%s under poison %d ended with status %d" % (family, byte, pr.returncode)
        pytest.fail(_dead_child + "\n" + tail)
    assert pr.returncode == 0, "%s under poison %d: exit status %d\n%s" % (family, byte, pr.returncode, tail)
    # the probe ran (it skips only without the variable) and no listed test skipped: a skip checks nothing
    summary = tail.strip().splitlines()[-1]
    assert "passed" in summary and "skipped" not in summary, summary
