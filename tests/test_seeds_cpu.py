"""The seeds of reads without a GPU: the yardstick of tests/seed_expect.py against its own slow definitions, the shared arithmetic
(csrc/fm_seeds.hpp) and the host-side plan (csrc/fm_seed_plan.hpp) as programs of their own under ASan + UBSan, the resources of the
kernels of csrc/fm_seeds.hip, and the argument checks of the C ABI that answer before a device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fm_expect as F
import sa_expect as A
import seed_expect as E
from gbwt_rs_amd import _lib, api
from test_merge_cpu import sanitized_program

SMALL = A.small_texts()


def window(text):
    """The containment definition is quadratic in the read and looks the text up for every pair: short windows of the long texts."""
    return text[:300] + text[-300:] if len(text) > 600 else text


@pytest.mark.parametrize("name,text", SMALL + [("mutated_rows", A.mutated_rows(4, 120, 3))], ids=[name for name, _ in SMALL] + ["mutated_rows"])
def test_rule_is_the_containment_definition(name, text):
    text = window(text)
    reads = [r for r in E.reads_of(text, rounds=2) if len(r) <= 77] + [text[:40], text[-40:]]
    assert len(reads) > 14
    for read in reads:
        for strand in (E.FORWARD, E.REVERSE):
            p = E.strand_read(read, strand)
            start = E.starts(text, p)
            assert start == E.starts_slow(text, p), (read, strand)
            assert all(a <= b for a, b in zip(start, start[1:])), (read, strand)         # the starts never decrease
            for min_length in (1, 5):
                assert E.seeds_by_rule(start, len(p), min_length) == E.seeds_by_containment(text, p, min_length), (read, strand, min_length)
            assert E.per_end_steps(text, p) <= len(p) * (len(p) + 3) // 2


def test_known_seeds():
    text = b"ACAC\0ACA\0"
    sa = F.suffix_array(text)
    assert sa.tolist() == [8, 4, 7, 2, 5, 0, 3, 6, 1]
    # ACACA: ACAC occurs at 0 and nowhere else, then CACA does not occur: ACA (twice) ends the read
    assert E.starts(text, b"ACACA") == [0, 0, 0, 0, 0, 2]
    assert E.expected(text, sa, b"ACACA", E.FORWARD) == [(0, 4, 1, 5, 6), (2, 5, 1, 4, 6)]
    # G splits the read; the endmarker is a byte like any other
    assert E.starts(text, b"CAGA\0A") == [0, 0, 0, 3, 3, 3, 4]
    assert E.expected(text, sa, b"CAGA\0A", E.FORWARD) == [(0, 2, 1, 7, 9), (3, 5, 1, 2, 3), (4, 6, 1, 1, 2)]
    assert E.seeds_by_rule(E.starts(text, b"ACACA"), 5, min_length=4) == [(0, 4)] and E.seeds_by_rule(E.starts(text, b"ACACA"), 5, min_length=0) == [(0, 4), (2, 5)]
    # the reverse strand: GTGT reads ACAC; lower case and other bytes
    assert E.reverse_complement(b"GTGT") == b"ACAC" and E.reverse_complement(b"acgtNx\0") == b"NNNACGT"
    assert E.expected(text, sa, b"GTGT", E.REVERSE) == [(0, 4, 2, 5, 6)] and E.expected(text, sa, b"GTGT", E.FORWARD) == []
    assert E.expected(text, sa, b"ZZ", E.FORWARD) == [] and E.expected(text, sa, b"", E.FORWARD) == []
    # steps of one search per end: ACACA -- 1, 2, 3, 4 and 3 + the failing one
    assert E.per_end_steps(text, b"ACACA") == 1 + 2 + 3 + 4 + 4
    assert E.per_end_steps(text, b"AZA") == 1 + 0 + 1                             # Z costs nothing, and nothing is tried across it
    assert E.anchored_steps_of_matching_read(150, 16) == 780 and E.anchored_steps_of_matching_read(16, 16) == 16 and E.anchored_steps_of_matching_read(17, 16) == 18
    assert api.reverse_complement(b"acgtNx\0") == b"NNNACGT" and api.reverse_complement("GATTACA") == b"TGTAATC"


SEED_CASES = (["complement_and_strands", "anchors"] +
              [f"{layout}_{case}" for layout in ("packed", "plain")
               for case in ("layout", "longest_suffix_at_every_end", "rule_is_containment", "anchored_plan_is_exact", "matching_read_searches_anchors_only", "absent_byte_mid_read")] +
              ["primary_row_inside_the_range", "empty_text"])
PLAN_CASES = ("constants", "no_reads", "slots_both_strands", "bytes_both_strands", "scratch_is_the_sum", "end_slots", "slots_one_strand", "hits", "short_reads", "capacity_exact_fit",
              "capacity_one_byte_short", "strands_outside_1_to_3", "reads_first_refused", "bytes_first_refused", "width_refused_before_memory")


def test_seed_arithmetic_under_sanitizers(tmp_path):
    """tests/cpp/fm_seeds.cpp: fm_longest_suffix over host-filled blocks of both layouts against naive substring search at read lengths 0, 1,
    K - 1, K, K + 1 and 2K + 1 on both strands, an absent byte mid-read, the primary row inside the range, and the anchored plan against the
    containment definition."""
    _, lines = sanitized_program(tmp_path, "fm_seeds")
    assert lines == ["ok " + case for case in SEED_CASES] + ["done"]


def test_seed_plan_under_sanitizers(tmp_path):
    """tests/cpp/fm_seed_plan.cpp: the slots and bytes of a request, an exact fit, one byte short, and the refusals."""
    _, lines = sanitized_program(tmp_path, "fm_seed_plan")
    assert lines == ["ok " + case for case in PLAN_CASES] + ["done"]


def test_seed_kernels_compile_without_scratch():
    """Every kernel of fm_seeds.hip for gfx950: nothing spilled, no scratch; the two search kernels within 64 VGPRs."""
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                          os.path.join(_lib.CSRC, "fm_seeds.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = {}
    for at, line in enumerate(lines):
        if "Function Name" in line and "k_seed_" in line:
            block = "\n".join(lines[at:at + 14])
            assert int(re.search(r"VGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"SGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)) == 0, block
            seen[re.search(r"\d+(k_seed_[a-z_]+?)E", line).group(1)] = int(re.search(r" VGPRs: (\d+)", block).group(1))
    assert sorted(seen) == ["k_seed_anchor_count", "k_seed_anchors", "k_seed_fill", "k_seed_flags", "k_seed_refine", "k_seed_refine_count"], sorted(seen)
    assert seen["k_seed_anchors"] <= 64 and seen["k_seed_refine"] <= 64, seen


def test_seed_argument_checks_answer_before_the_device():
    L = _lib.lib()
    offsets, descending = (C.c_uint64 * 3)(0, 1, 2), (C.c_uint64 * 3)(0, 2, 1)
    data, out_offsets, n_seeds, n_hits = (C.c_uint8 * 2)(65, 67), (C.c_uint64 * 3)(), C.c_uint64(9), C.c_uint64(9)
    seeds, hit_offsets = (_lib.FmSeed * 4)(), (C.c_uint64 * 5)()

    def options(min_length=1, strands=3, max_occurrences=0, flags=0, reserved=0):
        return C.byref(_lib.FmSeedOptions(min_length, strands, max_occurrences, flags, reserved))

    assert C.sizeof(_lib.FmSeed) == 32 == api.SEED_DTYPE.itemsize and C.sizeof(_lib.FmSeedOptions) == 24
    assert [api.SEED_DTYPE.fields[name][1] for name, _ in _lib.FmSeed._fields_] == [getattr(_lib.FmSeed, name).offset for name, _ in _lib.FmSeed._fields_]
    for call, front in ((L.gbwt_hip_fm_seeds, ()), (L.gbwt_hip_fm_seed_graph_positions, (None, None))):
        def host(offs, bytes_, opts, out, total_seeds, hit_offs=None, total_hits=C.byref(n_hits), seeds_=None, call=call, front=front):
            return call(None, *front, offs, bytes_, 2, opts, out, seeds_, 4 if seeds_ else 0, total_seeds, hit_offs, None, 0, total_hits)
        # null outputs first
        assert host(offsets, data, None, out_offsets, None) == _lib.BAD_ARGUMENT and b"null total" in L.gbwt_hip_last_error()
        assert host(offsets, data, None, None, C.byref(n_seeds)) == _lib.BAD_ARGUMENT and n_seeds.value == 0
        assert host(offsets, data, options(max_occurrences=5), out_offsets, C.byref(n_seeds), total_hits=None) == _lib.BAD_ARGUMENT and b"total of the hits" in L.gbwt_hip_last_error()
        assert host(offsets, data, options(max_occurrences=5), out_offsets, C.byref(n_seeds), None, C.byref(n_hits), seeds) == _lib.BAD_ARGUMENT and b"null hit offsets" in L.gbwt_hip_last_error()
        assert n_hits.value == 0
        # then the reads
        assert host(None, data, options(strands=7), out_offsets, C.byref(n_seeds)) == _lib.BAD_ARGUMENT and b"null pattern offsets" in L.gbwt_hip_last_error()
        assert host(descending, data, options(strands=7), out_offsets, C.byref(n_seeds)) == _lib.BAD_ARGUMENT and b"do not ascend at pattern 1" in L.gbwt_hip_last_error()
        assert host(offsets, None, options(strands=7), out_offsets, C.byref(n_seeds)) == _lib.BAD_ARGUMENT and b"null pattern bytes" in L.gbwt_hip_last_error()
        # then the options
        for strands in (0, 4):
            assert host(offsets, data, options(strands=strands, flags=1), out_offsets, C.byref(n_seeds)) == _lib.BAD_ARGUMENT and b"strands" in L.gbwt_hip_last_error()
        assert host(offsets, data, options(flags=1), out_offsets, C.byref(n_seeds)) == _lib.BAD_ARGUMENT and b"flags and reserved" in L.gbwt_hip_last_error()
        assert host(offsets, data, options(reserved=1), out_offsets, C.byref(n_seeds)) == _lib.BAD_ARGUMENT and b"flags and reserved" in L.gbwt_hip_last_error()
        # then the object
        hits_too = dict(hit_offs=hit_offsets)
        assert host(offsets, data, options(max_occurrences=5), out_offsets, C.byref(n_seeds), **hits_too) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()
        if not front:
            assert host(offsets, data, None, out_offsets, C.byref(n_seeds)) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()
        else:                                                                  # tags are hits: a request without any has nothing to tag
            assert host(offsets, data, options(), out_offsets, C.byref(n_seeds), **hits_too) == _lib.BAD_ARGUMENT and b"max_occurrences > 0" in L.gbwt_hip_last_error()
    rows = _lib.FmSeedRows()
    assert L.gbwt_hip_fm_seeds_device(None, offsets, data, 2, 2, None, None) == _lib.BAD_ARGUMENT and b"null output" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_seeds_device(None, None, data, 2, 2, None, C.byref(rows)) == _lib.BAD_ARGUMENT and b"null pattern offsets" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_seeds_device(None, offsets, data, 1 << 31, 2, None, C.byref(rows)) == _lib.BAD_ARGUMENT and b"too many patterns" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_seeds_device(None, offsets, data, 2, 2, options(strands=0), C.byref(rows)) == _lib.BAD_ARGUMENT and b"strands" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_seeds_device(None, offsets, data, 2, 2, None, C.byref(rows)) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_seed_graph_positions_device(None, None, None, offsets, data, 2, 2, options(max_occurrences=1), C.byref(rows)) == _lib.BAD_ARGUMENT
    assert b"null FM-index" in L.gbwt_hip_last_error() and rows.d_seeds is None and rows.total_seeds == 0
    assert L.gbwt_hip_fm_last_seed_info(None, C.byref(_lib.FmSeedInfo())) == _lib.BAD_ARGUMENT


def test_python_seed_arguments():
    assert (api.STRAND_FORWARD, api.STRAND_REVERSE, api.STRAND_BOTH) == (1, 2, 3)
    assert api.SEED_DTYPE.names == ("lo", "hi", "start", "end", "strand", "reserved")
    opts = api.FMIndex._seed_options(5, api.STRAND_REVERSE, 100)
    assert (opts.min_length, opts.strands, opts.max_occurrences, opts.flags, opts.reserved) == (5, 2, 100, 0, 0)
    for bad in ((1, 0, 0), (1, 4, 0), (-1, 3, 0), (1, 3, -1)):
        with pytest.raises(ValueError):
            api.FMIndex._seed_options(*bad)
    fm = api.FMIndex(None)                                                     # no object: the reads are looked at first
    for bad, error in ((b"ACGT", TypeError), ([5], TypeError), ((np.array([0, 2, 1]), b"ACG"), ValueError)):
        with pytest.raises(error):
            fm.seeds(bad)
    with pytest.raises(ValueError):
        fm.seeds([b"ACGT"], strands=0)
    with pytest.raises(ValueError):
        fm.seeds_device(0, 0, -1, 0)
    assert api.reverse_complement(b"") == b"" and api.reverse_complement(bytes(range(256))) == E.reverse_complement(bytes(range(256)))
