"""The decisions of a GFA lines request (csrc/lines_plan.hpp) without a GPU: tests/cpp/lines_plan.cpp as a program of its own under ASan + UBSan."""
from test_merge_cpu import sanitized_program

SHAPES = ("1_1", "1_2", "3_7", "1048576_2147483647")      # (rows, chunk bound)
CASES = tuple(kind + "_layout_" + shape for shape in SHAPES for kind in ("lines", "tokens")) + (
    "lines_layout_words", "tokens_layout_words", "scratch_at",
    "chunks_cap_total_0", "chunks_cap_below_a_chunk", "chunks_cap_a_chunk", "chunks_cap_above_a_chunk", "chunks_cap_last_served", "chunks_cap_first_refused",
    "chunks_cap_rows_alone", "refusal_texts",
    "sizing_cached", "sizing_plain", "sizing_translated", "sizing_translated_ignores_cache",
    "passes_default_with_ref", "passes_default_without_ref", "passes_pan_sn_with_ref", "passes_pan_sn_without_ref", "passes_ref_only_with_ref", "passes_ref_only_without_ref",
    "token_digits", "token_names",
    "batch_larger_than_budget_goes_alone", "batch_exact_fit", "batch_one_byte_over", "batch_last_short", "batch_without_lengths_by_count",
    "batch_beyond_the_lengths_estimates_0", "batch_first_always_goes_in")


def test_lines_plan_under_sanitizers(tmp_path):
    """Every case prints "ok <case>" (the expected values stand in the program, with the arithmetic that gives them); sanitized_program
    refuses a FAIL line, a sanitizer report (exit status) and a missing "done"."""
    _, lines = sanitized_program(tmp_path, "lines_plan")
    assert lines == ["ok " + case for case in CASES] + ["done"]
