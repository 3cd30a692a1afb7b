"""The memo of a request family (csrc/request_key.hpp) without a GPU: tests/cpp/request_key.cpp as a program of its own under ASan + UBSan."""
from test_merge_cpu import sanitized_program

CASES = ("fresh_matches_nothing", "fresh_not_even_empty", "empty_same_parameters", "empty_other_parameter", "empty_not_bytes", "equal_bytes_match",
         "one_parameter_differs", "prefix_shorter", "prefix_longer", "last_byte_differs", "null_with_length", "more_parts", "two_parts_match",
         "two_parts_other_split", "two_parts_as_one", "second_part_differs", "dropped_matches_nothing", "store_after_drop", "store_replaces",
         "null_parts_accepted")


def test_request_key_under_sanitizers(tmp_path):
    """Every case prints "ok <case>"; sanitized_program refuses a FAIL line, a sanitizer report (exit status) and a missing "done"."""
    _, lines = sanitized_program(tmp_path, "request_key")
    assert lines == ["ok " + case for case in CASES] + ["done"]
