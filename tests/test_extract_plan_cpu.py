"""The decisions of an extraction request (csrc/extract_plan.hpp) without a GPU: tests/cpp/extract_plan.cpp as a program of its own under ASan + UBSan."""
from test_merge_cpu import sanitized_program

CASES = ("summary_same_counts", "summary_counts_differ", "summary_invalid_id", "summary_first_without_samples", "summary_no_ids", "summary_no_sample_counts",
         "stride_below_half_a_million", "stride_from_half_a_million", "stride_by_size", "stride_capped", "stride_parts_divide_first", "stride_set", "stride_coarse_one",
         "headline_rows", "headline_walk", "headline_without_fused_offsets", "ragged_needs_order", "one_invalid_id",
         "parts_same_segments_sum", "parts_ragged", "uncut_no_samples", "uncut_segments_off", "uncut_2_to_31_rows",
         "defer_on", "defer_knob_off", "defer_all_valid", "defer_cannot_cut", "defer_invalid_id", "defer_counts_differ", "defer_no_rows_yet", "defer_parted",
         "unsegmented_pairs", "unsegmented_one_end", "unsegmented_paths_per_wave", "tuned_paths_per_wave",
         "lean_refuses_whole_rows", "lean_serves_empty_rows", "catch_up_lean", "catch_up_two", "catch_up_capped",
         "ring_holds_two_pieces", "ring_32_with_piece_16", "headroom_ring_minus_piece", "headroom_clamped_to_piece", "headroom_without_pieces",
         "gather_reach_511", "gather_reach_512", "gather_reach_no_records", "gather_reach_knob",
         "pool_blocks", "pool_blocks_size_below_sequences", "pool_paths_per_wave", "pool_paths_per_wave_tuned")


def test_extract_plan_under_sanitizers(tmp_path):
    """Every case prints "ok <case>" (the expected values stand in the program, with the arithmetic that gives them); sanitized_program
    refuses a FAIL line, a sanitizer report (exit status) and a missing "done"."""
    _, lines = sanitized_program(tmp_path, "extract_plan")
    assert lines == ["ok " + case for case in CASES] + ["done"]
