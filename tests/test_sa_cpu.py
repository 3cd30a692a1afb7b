"""Suffix arrays without a GPU: the yardsticks of tests/sa_expect.py against the brute-force sort of tests/tags_expect.py, the shared key
packing (csrc/sa_key.hpp) and the host-side plan (csrc/sa_plan.hpp) as programs of their own under ASan + UBSan, and the argument checks of
the C ABI that answer before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import sa_expect as A
import tags_expect as T
from gbwt_rs_amd import _lib
from test_merge_cpu import sanitized_program

SMALL = A.small_texts()


@pytest.mark.parametrize("name,text", SMALL, ids=[name for name, _ in SMALL])
def test_doubling_and_check_against_the_brute_force_sort(name, text):
    want = T.suffix_array(text)
    assert np.array_equal(A.doubling(text), want)
    assert A.check(text, want) is None
    if len(text) >= 2:
        assert A.check(text, want[::-1]) is not None


def test_check_rejects_swaps_duplicates_and_an_off_by_one():
    text = A.mutated_rows(6, 500, 3)
    sa = A.doubling(text)
    assert A.check(text, sa) is None and A.check(text, T.suffix_array(text)) is None
    for i in (0, 1, len(text) // 2, len(text) - 2):                       # a single adjacent swap anywhere
        bad = sa.copy()
        bad[i], bad[i + 1] = bad[i + 1], bad[i]
        assert "out of order" in A.check(text, bad), i
    bad = sa.copy()
    bad[7] = bad[8]
    assert "not a permutation" in A.check(text, bad)
    assert "out of range" in A.check(text, sa + np.uint64(1))             # off by one: the largest value leaves the text
    shifted = sa.copy()
    shifted[shifted > 0] -= np.uint64(1)                                  # off by one the other way: 0 twice
    assert "not a permutation" in A.check(text, shifted)
    assert "shape" in A.check(text, sa[:-1])
    assert A.check(b"", np.zeros(0, dtype=np.uint64)) is None


def test_bwt_and_runs():
    text = b"ACAC\0ACA\0"
    sa = T.suffix_array(text)
    assert sa.tolist() == [8, 4, 7, 2, 5, 0, 3, 6, 1]
    # T[7], T[3], T[6], T[1], T[4], the sentinel, T[2], T[5], T[0]
    assert A.bwt(text, sa, 36).tobytes() == b"ACCC\0$AAA" and A.runs(A.bwt(text, sa, 36)) == 5
    assert A.bwt(text, sa, 0).tobytes() == b"ACCC\0\0AAA" and A.runs(A.bwt(text, sa, 0)) == 4
    assert A.runs(A.bwt(b"", [])) == 0 and A.runs(A.bwt(b"A", [0], 255)) == 1


KEY_CASES = ("strings_of_length_0_to_3", "short_strings_alone", "short_strings_against_each_other", "tail_with_zeros", "tail_of_a_run", "tail_of_zeros", "tail_of_255",
             "periodic_with_endmarker", "key_layout_full", "key_layout_tail", "rank_bits", "round_key", "round_key_group_first", "second_rank")
PLAN_CASES = ("n_0_succeeds_without_memory", "widths_n_1", "widths_n_3000060", "small_text_smallest_buffers", "bytes_per_phase", "peak_is_49_bytes_per_position",
              "capacity_exact_fit", "capacity_one_byte_short", "width_last_served", "width_first_refused", "width_refused_before_memory", "width_last_served_still_needs_memory")


def test_key_order_under_sanitizers(tmp_path):
    """tests/cpp/sa_key.cpp: the first keys order all byte strings of length <= 3 over {0, 1, 255} and the tails of texts as the suffixes
    themselves are ordered, and the word form of the key (the kernel's) is the byte form."""
    _, lines = sanitized_program(tmp_path, "sa_key")
    assert lines == ["ok " + case for case in KEY_CASES] + ["done"]


def test_plan_under_sanitizers(tmp_path):
    """tests/cpp/sa_plan.cpp: the refusals at 2^32 - 2 / 2^32 - 1 positions and one byte short of the peak, n = 0, and the bytes per phase."""
    _, lines = sanitized_program(tmp_path, "sa_plan")
    assert lines == ["ok " + case for case in PLAN_CASES] + ["done"]


def test_argument_checks_answer_before_the_device():
    L = _lib.lib()
    byte, word, runs = (C.c_uint8 * 1)(), (C.c_uint64 * 1)(), C.c_uint64(7)
    for call, more in ((L.gbwt_hip_suffix_array_text, ()), (L.gbwt_hip_suffix_array_text_device, (None,))):
        assert call(0, byte, 1, 256, word, None, *more, C.byref(runs)) == _lib.BAD_ARGUMENT and runs.value == 0
        assert call(0, byte, 1, -1, word, None, *more, None) == _lib.BAD_ARGUMENT
        assert call(0, None, 1, 0, word, None, *more, None) == _lib.BAD_ARGUMENT
        assert call(0, byte, 1, 0, None, None, *more, None) == _lib.BAD_ARGUMENT
        # the width is refused before any byte is read (nothing stands behind these pointers) and before a device is asked for
        assert call(0, byte, (1 << 32) - 1, 0, word, None, *more, None) == _lib.UNSUPPORTED
        assert b"2^32 - 2" in L.gbwt_hip_last_error()
        assert call(0, None, 0, 0, None, None, *more, C.byref(runs)) == _lib.OK and runs.value == 0        # an empty text: nothing to do
    info = _lib.SuffixArrayInfo()
    assert L.gbwt_hip_last_suffix_array_info(None, C.byref(info)) == _lib.OK and info.n == 0 and info.rounds == 0
    assert L.gbwt_hip_last_suffix_array_info(None, None) == _lib.BAD_ARGUMENT
    out = _lib.SuffixArray()
    assert L.gbwt_hip_path_suffix_array_device(None, None, None, 0, 0, C.byref(out)) == _lib.BAD_ARGUMENT
    assert L.gbwt_hip_write_suffix_array(None, None, b"x", None) == _lib.BAD_ARGUMENT
