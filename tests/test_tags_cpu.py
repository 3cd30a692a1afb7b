"""gbz-extract's `tag-array` mode without a GPU: the C ABI declares, exports and types the entry points, the kernels compile for gfx950
without scratch, and the yardstick of tests/test_gpu_tags.py (tests/tags_expect.py) is pinned: the known answer of example.gbz, the
reference's two sorts against the gather, and a true suffix array of the example text with its runs counted by hand."""
import os
import re
import subprocess

import numpy as np

from gbwt_rs_amd import _lib
import seq_expect as E
import tags_expect as T
from test_merge_cpu import sanitized_program

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_SYMBOLS = ["gbwt_hip_tags_device", "gbwt_hip_tags", "gbwt_hip_write_tag_array", "gbwt_hip_last_tags_ms"]


def example():
    gfa = open(os.path.join(GOLDEN, "example.gfa"), "rb").read()
    table = E.LabelTable.from_gfa(gfa)
    rows = T.gfa_rows(gfa)                      # P-lines A, B, then the four W-lines: path ids 0 .. 5
    return table, rows


def test_entry_points_declared_exported_and_typed():
    header = open(_lib.HEADER).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"gbwt_hip_status\s+" + name + r"\(", header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    from gbwt_rs_amd import GBZ
    for method in ("tag_array", "tags_device", "write_tag_array", "text_length", "last_tags_ms"):
        assert callable(getattr(GBZ, method)), method


def test_tag_kernels_compile_without_scratch():
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                          os.path.join(_lib.CSRC, "tags.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = {}
    for at, line in enumerate(lines):
        if "Function Name" in line and "k_tag" in line:
            block = "\n".join(lines[at:at + 14])
            assert int(re.search(r"VGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)) == 0, block
            seen[line.split("Function Name: ")[1].split()[0]] = int(re.search(r"VGPRs: (\d+)", block).group(1))
    gather = [name for name in seen if "6k_tagsI" in name]
    assert len(gather) == 2, seen               # 32-bit and 64-bit hints
    assert all(seen[name] <= 64 for name in gather), seen     # eight waves per SIMD


def test_extract_files_under_sanitizers(tmp_path):
    """tests/cpp/extract_files.cpp: the files between gbz-extract's three modes (csrc/extract_files.hpp) on the host.  Every case prints
    "ok <case>"; sanitized_program refuses a FAIL line, a sanitizer report (exit status) and a missing "done"."""
    _, lines = sanitized_program(tmp_path, "extract_files")
    assert lines == ["ok " + case for case in (
        "writer_line_format", "writer_line_parses_back_names_with_spaces", "two_fields_no_final_newline", "crlf_stripped", "empty_text", "line_without_tab",
        "empty_line_in_the_middle", "newline_alone", "non_digit_in_id", "non_digit_in_bases", "empty_id_field", "twenty_digits", "nineteen_nines", "file_that_does_not_exist",
        "path_exists_half_of_sequences", "path_exists_2_63", "path_exists_2_64_minus_1", "path_exists_last_id", "no_such_path_message", "length_mismatch_message",
        "matching_lengths", "endmarker_argument")] + ["done"]


def test_example_known_answer():
    table, rows = example()
    assert table.len[[11, 12, 13, 14, 15, 16, 17, 21, 22, 23, 24, 25]].tolist() == [1] * 12
    text, offsets = T.tag_text(table.len, rows)
    assert np.diff(offsets).tolist() == [6, 5, 6, 6, 6, 5]                     # len = 5, 4, 5, 5, 5, 4 and an endmarker each
    assert offsets.tolist() == [0, 6, 11, 17, 23, 29, 34]
    assert text.size == 34
    assert text[0:6].tolist() == [22528, 24576, 28672, 30720, 34816, 0]        # nodes 11, 12, 14, 15, 17 forward, the endmarker
    assert text[23:29].tolist() == [43008, 45056, 49152, 48128, 44032, 0]      # >21>22>24<23<21
    assert text[23:29].tolist() == [21 << 11, 22 << 11, 24 << 11, (23 << 11) | 1024, (21 << 11) | 1024, 0]
    # the paths in another order, one twice: rows move, tags do not change
    order = [5, 0, 5]
    moved, moved_offsets = T.tag_text(table.len, [rows[p] for p in order])
    assert moved_offsets.tolist() == [0, 5, 11, 16]
    assert moved.tolist() == text[29:34].tolist() + text[0:6].tolist() + text[29:34].tolist()


def test_offsets_inside_long_labels_and_the_carry():
    """w counts in reading direction and is ADDED: behind 1 024 bases it carries into the orientation bit, as in the reference."""
    lengths = np.zeros(8, dtype=np.int64)
    lengths[3], lengths[5] = 3, 1030
    text, offsets = T.tag_text(lengths, [np.array([2 * 3 + 1, 2 * 5], dtype=np.uint64)])
    assert offsets.tolist() == [0, 1034]
    assert text[:3].tolist() == [(3 << 11) + 1024, (3 << 11) + 1025, (3 << 11) + 1026]
    assert text[3] == 5 << 11 and text[3 + 1023] == (5 << 11) + 1023
    assert text[3 + 1024] == (5 << 11) | 1024 and text[3 + 1029] == (5 << 11) + 1029 and text[-1] == 0


def test_two_sorts_equal_the_gather_for_permutations():
    table, rows = example()
    text, _ = T.tag_text(table.len, rows)
    for seed in range(20):
        sa = np.random.default_rng(seed).permutation(text.size).astype(np.uint64)
        assert np.array_equal(T.two_sorts(text, sa), T.gather(text, sa)), seed
    # a longer text with long labels
    lengths = np.random.default_rng(99).integers(1, 1025, size=64)
    big_rows = [np.random.default_rng(k).integers(2, 128, size=50).astype(np.uint64) for k in range(7)]
    big, _ = T.tag_text(lengths, big_rows)
    sa = np.random.default_rng(5).permutation(big.size).astype(np.uint64)
    assert np.array_equal(T.two_sorts(big, sa), T.gather(big, sa))
    assert T.runs(T.gather(big, np.arange(big.size))) == big.size               # in text order no two neighbours share a tag (labels of at most 1 024 bases)
    assert T.runs(np.zeros(0, dtype=np.uint64)) == 0 and T.runs(np.array([7, 7, 7])) == 1 and T.runs(np.array([0, 1, 1, 0])) == 3


def test_true_suffix_array_of_the_example_text():
    table, rows = example()
    text, _ = T.tag_text(table.len, rows)
    _, data = E.expected_rows(table, [(r >> np.uint64(1), (r & np.uint64(1)).astype(bool)) for r in rows], 0)
    assert data == b"GATAA\x00GATA\x00GATAA\x00GTTCA\x00GATAC\x00GATA\x00"
    sa = T.suffix_array(data)
    assert sorted(sa.tolist()) == list(range(34))
    assert sa[:6].tolist() == [33, 28, 5, 10, 22, 16]                           # the endmarkers: shorter suffixes first
    assert all(data[int(a):] < data[int(b):] for a, b in zip(sa[:-1], sa[1:]))
    tags = T.gather(text, sa)
    assert np.array_equal(tags, T.two_sorts(text, sa))
    assert tags.tolist() == [0, 0, 0, 0, 0, 0, 51200, 34816, 51200, 34816, 34816, 30720, 30720, 48128, 45056, 45056, 24576, 24576, 45056, 44032, 32768, 43008,
                             43008, 22528, 22528, 43008, 22528, 49152, 49152, 28672, 28672, 49152, 28672, 26624]
    # counted by hand on the array above: 0 x 6 | 51200 | 34816 | 51200 | 34816 x 2 | 30720 x 2 | 48128 | 45056 x 2 | 24576 x 2 | 45056 | 44032 | 32768 |
    # 43008 x 2 | 22528 x 2 | 43008 | 22528 | 49152 x 2 | 28672 x 2 | 49152 | 28672 | 26624
    assert T.runs(tags) == 21
