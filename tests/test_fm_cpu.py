"""The FM-index without a GPU: the yardstick of tests/fm_expect.py against its own definition, the shared layout (csrc/fm_layout.hpp) and
the host-side plan (csrc/fm_plan.hpp) as programs of their own under ASan + UBSan, and the argument checks of the C ABI that answer before
a device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fm_expect as F
import sa_expect as A
from gbwt_rs_amd import _lib, api
from test_merge_cpu import sanitized_program

SMALL = A.small_texts()


@pytest.mark.parametrize("name,text", SMALL, ids=[name for name, _ in SMALL])
def test_fast_occurrences_are_the_definition_and_stand_together(name, text):
    text = text[:600] + text[-600:] if len(text) > 1200 else text
    sa = F.suffix_array(text)
    patterns = F.text_patterns(text)
    assert len(patterns) % 64 != 0
    ranges, rows = F.expected(text, sa, patterns)
    for p, (lo, hi), row in zip(patterns, ranges, rows):
        slow = F.occurrences_slow(text, p)
        assert np.array_equal(F.occurrences(text, p), slow), p
        assert hi - lo == slow.size and sorted(row.tolist()) == slow.tolist(), p
    assert tuple(ranges[0]) == (0, len(text))                                  # the empty pattern
    assert tuple(ranges[patterns.index(text + b"A")]) == (0, 0)


def test_known_ranges():
    text = b"ACAC\0ACA\0"
    sa = F.suffix_array(text)
    assert sa.tolist() == [8, 4, 7, 2, 5, 0, 3, 6, 1]
    ranges, rows = F.expected(text, sa, [b"A", b"AC", b"ACA", b"\0", b"C", b"CA\0", b"G", b""])
    assert ranges.tolist() == [[2, 6], [3, 6], [4, 6], [0, 2], [6, 9], [7, 8], [0, 0], [0, 9]]
    assert rows[1].tolist() == [2, 5, 0] and rows[5].tolist() == [6] and rows[6].tolist() == []
    with pytest.raises(AssertionError):                                        # rows 0 and 7 swapped: the suffixes that start with C are apart
        F.sa_range(np.array([6, 4, 7, 2, 5, 0, 3, 8, 1]), F.occurrences(text, b"C"))


LAYOUT_CASES = (["count_prefixes_0_to_256", "block_arithmetic", "empty_text", "text_C_pattern_C"] +
                [f"sigma_{s}_length_{n}" for s, b in ((1, 96), (6, 96), (256, 256)) for n in (b - 1, b, b + 1, 2 * b, 2 * b + 1)] +
                [f"{layout}_primary_{where}" for layout in ("packed", "plain") for where in ("first_in_block", "last_in_block", "row_0")] +
                ["one_symbol_primary_row_95", "one_symbol_primary_row_96"])
PLAN_CASES = ("n_0", "table_and_histogram_bytes", "packed_sizes", "packed_index_and_scratch", "packed_block_edges", "count_only_and_own_suffix_array", "plain_sizes", "plain_from_sigma_9",
              "packed_bytes_per_position", "plain_bytes_per_position", "capacity_exact_fit", "capacity_one_byte_short", "width_last_served", "width_first_refused",
              "width_refused_before_memory", "width_last_served_still_needs_memory")


def test_layout_under_sanitizers(tmp_path):
    """tests/cpp/fm_layout.cpp: blocks filled on the host through fm_layout.hpp; rank at every row and whole backward searches against naive
    counts, for one, six and 256 symbols at the block edges, a sentinel that equals a text byte, and the primary row first in a block, last
    in a block and at SA row 0."""
    _, lines = sanitized_program(tmp_path, "fm_layout")
    assert lines == ["ok " + case for case in LAYOUT_CASES] + ["done"]


def test_plan_under_sanitizers(tmp_path):
    """tests/cpp/fm_plan.cpp: the sizes of both layouts, the refusals at 2^32 - 1 positions and one byte short of the peak."""
    _, lines = sanitized_program(tmp_path, "fm_plan")
    assert lines == ["ok " + case for case in PLAN_CASES] + ["done"]


def test_kernels_compile_without_scratch():
    """Every kernel of fm_index.hip for gfx950: nothing spilled, no scratch; the search kernel within 64 VGPRs."""
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                          os.path.join(_lib.CSRC, "fm_index.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = {}
    for at, line in enumerate(lines):
        if "Function Name" in line and "k_fm_" in line:
            block = "\n".join(lines[at:at + 14])
            assert int(re.search(r"VGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"SGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)) == 0, block
            seen[re.search(r"\d+(k_fm_[a-z_]+?)E", line).group(1)] = int(re.search(r" VGPRs: (\d+)", block).group(1))
    assert sorted(seen) == ["k_fm_block_counts_packed", "k_fm_block_counts_plain", "k_fm_codes", "k_fm_compact", "k_fm_count", "k_fm_fill_packed", "k_fm_fill_plain", "k_fm_histogram",
                            "k_fm_locate_fill", "k_fm_narrow_sa", "k_fm_run_flags"], sorted(seen)
    assert seen["k_fm_count"] <= 64, seen


def test_argument_checks_answer_before_the_device():
    L = _lib.lib()
    byte, handle = (C.c_uint8 * 1)(), C.c_void_p(5)
    # builds: the output, the sentinel, the flags and the width are looked at before a device is asked for
    for call, more in ((L.gbwt_hip_fm_build_text, ()), (L.gbwt_hip_fm_build_text_device, (None,))):
        def build(text, n, sentinel, flags, out, call=call, more=more):
            tail = (None,) if more else ()                                     # the stream of the device form
            return call(0, text, n, sentinel, *more, flags, *tail, out)
        assert build(byte, 1, 0, 0, None) == _lib.BAD_ARGUMENT
        assert build(byte, 1, 256, 0, C.byref(handle)) == _lib.BAD_ARGUMENT and handle.value is None
        assert build(byte, 1, -1, 0, C.byref(handle)) == _lib.BAD_ARGUMENT
        assert build(byte, 1, 0, 2, C.byref(handle)) == _lib.BAD_ARGUMENT and b"GBWT_HIP_FM_COUNT_ONLY" in L.gbwt_hip_last_error()
        assert build(None, 1, 0, 0, C.byref(handle)) == _lib.BAD_ARGUMENT
        assert build(byte, (1 << 32) - 1, 0, 0, C.byref(handle)) == _lib.UNSUPPORTED and b"2^32 - 2" in L.gbwt_hip_last_error()
        assert build(byte, (1 << 32) - 1, 0, _lib.FM_COUNT_ONLY, C.byref(handle)) == _lib.UNSUPPORTED
    assert L.gbwt_hip_path_fm_index(None, None, None, 0, 0, 0, C.byref(handle)) == _lib.BAD_ARGUMENT
    assert L.gbwt_hip_path_fm_index(None, None, None, 0, 0, 0, None) == _lib.BAD_ARGUMENT
    L.gbwt_hip_fm_close(None)
    assert L.gbwt_hip_fm_info(None, C.byref(_lib.FmIndexInfo())) == _lib.BAD_ARGUMENT
    # queries: null outputs and offsets that do not ascend are refused before the object is looked at
    offsets, descending = (C.c_uint64 * 3)(0, 1, 2), (C.c_uint64 * 3)(0, 2, 1)
    data, ranges, total = (C.c_uint8 * 2)(65, 67), (C.c_uint64 * 4)(), C.c_uint64(9)
    assert L.gbwt_hip_fm_count(None, offsets, data, 2, None) == _lib.BAD_ARGUMENT and b"null ranges" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_count(None, descending, data, 2, ranges) == _lib.BAD_ARGUMENT and b"do not ascend at pattern 1" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_count(None, None, data, 2, ranges) == _lib.BAD_ARGUMENT and b"null pattern offsets" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_count(None, offsets, None, 2, ranges) == _lib.BAD_ARGUMENT and b"null pattern bytes" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_count(None, offsets, data, 2, ranges) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()
    for call, front in ((L.gbwt_hip_fm_locate, ()), (L.gbwt_hip_fm_graph_positions, (None, None))):
        tail = (1,) if front else ()                                           # unique
        assert call(None, *front, offsets, data, 2, *tail, ranges, None, 0, None) == _lib.BAD_ARGUMENT and b"null total" in L.gbwt_hip_last_error()
        assert call(None, *front, offsets, data, 2, *tail, None, None, 0, C.byref(total)) == _lib.BAD_ARGUMENT and total.value == 0
        assert call(None, *front, descending, data, 2, *tail, ranges, None, 0, C.byref(total)) == _lib.BAD_ARGUMENT and b"do not ascend" in L.gbwt_hip_last_error()
        assert call(None, *front, offsets, data, 2, *tail, ranges, None, 0, C.byref(total)) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()
    out = _lib.FmLocated()
    assert L.gbwt_hip_fm_count_device(None, None, None, 0, 0, None) == _lib.BAD_ARGUMENT
    assert L.gbwt_hip_fm_locate_device(None, None, None, 1, 0, C.byref(out)) == _lib.BAD_ARGUMENT and b"null pattern offsets" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_graph_positions_device(None, None, None, offsets, data, 1 << 31, 2, 0, C.byref(out)) == _lib.BAD_ARGUMENT and b"too many patterns" in L.gbwt_hip_last_error()


def test_python_pattern_arguments():
    offsets, data = api._patterns_csr([b"AC", "G", b""])
    assert offsets.tolist() == [0, 2, 3, 3] and data.tobytes() == b"ACG"
    offsets, data = api._patterns_csr((np.array([0, 2, 3]), b"ACG"))
    assert offsets.dtype == np.uint64 and data.tobytes() == b"ACG"
    assert api._patterns_csr([])[0].tolist() == [0]
    for bad, error in ((b"ACGT", TypeError), ("ACGT", TypeError), ([5], TypeError), ((np.array([0, 2, 1]), b"ACG"), ValueError), ((np.array([0, 4]), b"ACG"), ValueError),
                       ((np.zeros(0), b""), ValueError)):
        with pytest.raises(error):
            api._patterns_csr(bad)
    with pytest.raises(ValueError):
        api.FMIndex.from_text(np.zeros((2, 2), dtype=np.uint8))
