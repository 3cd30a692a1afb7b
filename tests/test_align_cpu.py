"""The alignments of chains without a GPU: the yardstick of tests/align_expect.py against its own slow definition and the figures of the
definition, the shared arithmetic (csrc/fm_align.hpp) and the host-side plan (csrc/fm_align_plan.hpp) as programs of their own under ASan +
UBSan, the resources of the kernels of csrc/fm_align.hip, and the argument checks of the C ABI that answer before a device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import align_expect as AE
import chain_expect as X
import fm_expect as F
import fm_path_graphs as PG
import seed_expect as E
from gbwt_rs_amd import _lib, api
from test_chains_cpu import SETTINGS, case_reads, case_text
from test_merge_cpu import sanitized_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOST = 1 << 20


def rows_of(out, a):
    return out["alignments"][a], out["cigars"][out["cigar_offsets"][a]:out["cigar_offsets"][a + 1]]


def best_forward(out, k):
    for a in range(out["read_offsets"][k], out["read_offsets"][k + 1]):
        if out["alignments"][a][6] == E.FORWARD:
            return rows_of(out, a)
    return None


def test_the_two_forms_agree_on_the_first_case():
    text, sa = case_text()
    reads = case_reads(text)
    statuses = set()
    for setting in SETTINGS:
        slow = AE.expected_rows(text, sa, reads, 5, E.BOTH, MOST, *setting, band=8, form=AE.align_slow)
        fast = AE.expected_rows(text, sa, reads, 5, E.BOTH, MOST, *setting, band=8, form=AE.align)
        for key in ("read_offsets", "alignments", "cigar_offsets", "cigars", "wide", "unreachable", "cells"):
            assert slow[key] == fast[key], (setting, key)
        assert len(slow["alignments"]) == len(slow["chain_rows"]["chains"]) == slow["read_offsets"][-1]      # every chain is considered: one row each
        assert [row[2] for row in slow["alignments"]] == list(range(len(slow["alignments"])))
        statuses |= {row[5] for row in slow["alignments"]}
    assert statuses >= {AE.OK, AE.NONE}


def test_known_alignments_of_the_first_case():
    """The figures the definition gives for the best forward chains of reads 0 - 3: the device tests compare against the same yardstick."""
    text, sa = case_text()
    reads = case_reads(text)
    out = AE.expected_rows(text, sa, reads, 5, E.BOTH, MOST, 1000, 50, 1, 1, band=8, form=AE.align_slow)
    known = [(0, "150=", 10, 160), (2, "40=1X49=1X59=", 20, 170), (3, "69=3D78=", 30, 180), (5, "64=2I2=1I3=1I1=1I80=", 30, 180)]
    for k, (distance, cigar, start, end) in enumerate(known):
        row, entries = best_forward(out, k)
        assert (row[3], AE.cigar_string(entries), row[0], row[1], row[5]) == (distance, cigar, start, end, AE.OK), k
        assert api.cigar_string(entries) == cigar
    # read 3 shows the direction preference: the five inserted bases ACGTA partly match the text, and the diagonal goes first on a tie
    assert reads[3][70:75] == b"ACGTA" and AE.cigar_string(best_forward(out, 3)[1]).count("I") == 4
    # max_alignments 1: the best chain of every item only
    first = AE.expected_rows(text, sa, reads, 5, E.BOTH, MOST, 1000, 50, 1, 1, band=8, max_alignments=1)
    assert all(first["read_offsets"][k + 1] - first["read_offsets"][k] <= 2 for k in range(len(reads))) and best_forward(first, 3) == best_forward(out, 3)
    assert first["read_offsets"][6:] == [first["read_offsets"][6]] * 4


def test_overhang_two_pieces_and_ties():
    text, _ = case_text()
    n = len(text)
    # a read that runs over the end of the text: the band must reach the insertions
    read = text[-100:] + b"CATCATCATCATCATCATCA"
    assert len(read) == 120
    for band in (8, 19):
        assert AE.align_slow(read, text, [(n - 100, 0, 100)], band, 0, 0, n)[:1] + AE.align_slow(read, text, [(n - 100, 0, 100)], band, 0, 0, n)[2:] == (AE.NONE, AE.INF, 0, 0, [])
    status, width, distance, start, end, entries = AE.align_slow(read, text, [(n - 100, 0, 100)], 20, 0, 0, n)
    assert (status, width, distance, start, end, AE.cigar_string(entries)) == (AE.OK, 41, 20, n - 100, n, "100=20I")
    assert AE.align(read, text, [(n - 100, 0, 100)], 20, 0, 0, n) == (status, width, distance, start, end, entries)
    # the two pieces: diagonals 5 and 145
    pieces = text[5:60] + text[200:260]
    members = [(5, 0, 55), (200, 55, 60)]
    assert AE.band_of(members, 8) == (-3, 157)
    assert AE.align_slow(pieces, text, members, 8, 128, 0, n) == (AE.WIDE, 157, AE.INF, 0, 0, [])
    status, width, distance, start, end, entries = AE.align_slow(pieces, text, members, 8, 256, 0, n)
    assert (status, width) == (AE.OK, 157) and AE.align(pieces, text, members, 8, 256, 0, n) == (status, width, distance, start, end, entries)
    AE.check_alignment(pieces, text, (status, width, distance, start, end), entries)
    assert end == 260 and AE.cigar_string(entries).endswith("=") and distance < 55       # the free start: the first piece is cheaper misaligned than 140 deletions are
    # a periodic text: several ends tie, the smallest is taken
    periodic = PG.periodic([40]).text([0])
    assert periodic == b"AC" * 40 + b"\0"
    hi = len(periodic) - 1
    for form in (AE.align_slow, AE.align):
        status, width, distance, start, end, entries = form(b"ACACAC", periodic, [(10, 0, 6)], 4, 0, 0, hi)
        assert (status, width, distance, start, end, AE.cigar_string(entries)) == (AE.OK, 9, 0, 6, 12, "6=")         # ends 12, 14, 16, 18 and 20 all give 0
        status, width, distance, start, end, entries = form(PG.PERIODIC_READ, periodic, [(10, 0, 6), (16, 7, 6)], 4, 0, 0, hi)
        assert (status, width, distance, start, end, AE.cigar_string(entries)) == (AE.OK, 10, 1, 6, 18, "6=1I6=")       # the G is inserted; the ends 18 .. 28 tie
        AE.check_alignment(PG.PERIODIC_READ, periodic, (status, width, distance, start, end), entries)
    # bounds: the same chain inside a segment that ends early
    assert AE.align_slow(b"ACACAC", periodic, [(10, 0, 6)], 4, 0, 0, 13)[:5] == (AE.OK, 9, 0, 6, 12)
    assert AE.align_slow(b"ACACAC", periodic, [(10, 0, 6)], 1, 0, 0, 13)[0] == AE.NONE                  # ends 15 .. 17 lie beyond 13


ALIGN_CASES = ("edits", "high", "below", "below_start", "bounded", "none", "width_1", "width_63", "width_64", "width_65", "width_128", "width_129", "width_most", "wide", "wide_default")
PLAN_CASES = ("constants", "tile", "cigar_bound", "nothing", "item_bytes", "alignment_bytes", "direction_cigar_temp_words", "scratch_is_the_sum", "few", "capacity_exact_fit",
              "capacity_one_byte_short", "alignments_refused_before_memory", "most_alignments")


def test_align_arithmetic_under_sanitizers(tmp_path):
    """tests/cpp/fm_align.cpp: the rows of the DP with the functions of fm_align.hpp over host arrays -- a member above 2^32 - 200, a band below
    text position 0, bounds inside the text, W of 1, 63, 64, 65, 128, 129 and the most -- against the yardstick over the inputs the program prints."""
    got, lines = sanitized_program(tmp_path, "fm_align")
    numbers = lambda key: [int(v) for v in got.get(key, "").split()]
    assert [line.split(".")[0] for line in lines if ".options" in line] == list(ALIGN_CASES)
    widths, statuses = {}, {}
    for case in ALIGN_CASES:
        band, max_width, lo, hi, base = numbers(case + ".options")
        read, text = bytes(numbers(case + ".read")), bytes(numbers(case + ".text"))
        members = [tuple(int(v) for v in m.split(",")) for m in got[case + ".members"].split()]
        shifted = [(y - base, x, w) for y, x, w in members]
        status, width, distance, start, end, entries = AE.align_slow(read, text, shifted, band, max_width, lo - base, hi - base)
        if status == AE.OK:
            start, end = start + base, end + base
        assert numbers(case + ".result") == [status, width, distance, start, end], case
        assert numbers(case + ".cigar") == entries, case
        widths[case], statuses[case] = width, status
    assert [widths["width_" + w] for w in ("1", "63", "64", "65", "128", "129", "most")] == [1, 63, 64, 65, 128, 129, 1024]
    assert statuses["wide"] == statuses["wide_default"] == AE.WIDE and statuses["none"] == AE.NONE and widths["wide"] == 1024 and widths["wide_default"] == 257
    assert all(statuses[case] == AE.OK for case in ALIGN_CASES if case not in ("wide", "wide_default", "none"))
    assert max(y for y, _, _ in (tuple(int(v) for v in m.split(",")) for m in got["high.members"].split())) > (1 << 32) - 200
    assert numbers("high.result")[3] < 1 << 32 < numbers("high.result")[4] and numbers("high.result")[2] == numbers("edits.result")[2] == 6
    assert numbers("below.options")[0] == 8 and min(y - x for y, x, _ in [tuple(int(v) for v in m.split(",")) for m in got["below.members"].split()]) - 8 < 0
    assert AE.cigar_string(numbers("below_start.cigar")).endswith("I60=") or "I" in AE.cigar_string(numbers("below_start.cigar"))
    assert numbers("entry") == [(150 << 4) | 7, (1 << 4) | 8, 0xFFFFFFF1] and numbers("tile") == [8192, 1, 0]


def test_align_plan_under_sanitizers(tmp_path):
    """tests/cpp/fm_align_plan.cpp: the bytes of the scratch against hand-computed sizes, an exact fit, one byte short, nothing to do, and the refusal."""
    _, lines = sanitized_program(tmp_path, "fm_align_plan")
    assert lines == ["ok " + case for case in PLAN_CASES] + ["done"]


def test_align_kernels_compile_without_scratch():
    """Every kernel of fm_align.hip for gfx950: nothing spilled, no scratch; the DP at four waves a SIMD and 4 x (8192 + 1536) bytes of LDS a workgroup."""
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                          os.path.join(_lib.CSRC, "fm_align.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = {}
    for at, line in enumerate(lines):
        if "Function Name" in line and "k_align_" in line:
            block = "\n".join(lines[at:at + 14])
            assert int(re.search(r"VGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"SGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)) == 0, block
            seen[re.search(r"\d+(k_align_[a-z_]+?)E", line).group(1)] = (int(re.search(r" VGPRs: (\d+)", block).group(1)), int(re.search(r"LDS Size \[bytes/block\]: (\d+)", block).group(1)))
    assert sorted(seen) == ["k_align_dp", "k_align_rows", "k_align_select", "k_align_setup"], sorted(seen)
    assert seen["k_align_dp"][0] <= 128 and seen["k_align_dp"][1] == 4 * (8192 + 1536), seen
    makefile = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert re.search(r"^KERNELS = .*\bfm_align\b", makefile, re.M) and "capi_fm_align.o" in makefile


def test_align_symbols_in_the_header_and_the_library():
    header = open(os.path.join(ROOT, "include", "gbwt_hip.h")).read()
    L = _lib.lib()
    for name in ("gbwt_hip_fm_alignments", "gbwt_hip_fm_alignments_device", "gbwt_hip_fm_last_align_info", "gbwt_hip_fm_set_text", "gbwt_hip_fm_set_text_device",
                 "gbwt_hip_fm_keep_path_text"):
        assert re.search(r"gbwt_hip_status " + name + r"\(", header) and getattr(L, name)
    for name in ("gbwt_hip_fm_align_options", "gbwt_hip_fm_alignment", "gbwt_hip_fm_align_info", "gbwt_hip_fm_alignment_rows"):
        assert re.search(r"\} " + name + r";", header), name
    assert "Alignments of chains" in header and header.index("Alignments of chains") > header.index("Chains of seeds")
    assert [int(re.search(r"#define GBWT_HIP_ALIGN_" + name + r" (\d)u", header).group(1)) for name in ("OK", "WIDE", "NONE")] == [_lib.ALIGN_OK, _lib.ALIGN_WIDE, _lib.ALIGN_NONE] == [0, 1, 2]
    assert C.sizeof(_lib.FmAlignOptions) == 24 and C.sizeof(_lib.FmAlignment) == 40 == api.ALIGNMENT_DTYPE.itemsize
    assert [api.ALIGNMENT_DTYPE.fields[name][1] for name, _ in _lib.FmAlignment._fields_] == [getattr(_lib.FmAlignment, name).offset for name, _ in _lib.FmAlignment._fields_]
    assert api.ALIGNMENT_DTYPE.names == tuple(name for name, _ in _lib.FmAlignment._fields_)


def test_align_argument_checks_answer_before_the_device():
    L = _lib.lib()
    offsets, descending = (C.c_uint64 * 3)(0, 1, 2), (C.c_uint64 * 3)(0, 2, 1)
    data, out_offsets, n_rows, n_cigars = (C.c_uint8 * 2)(65, 67), (C.c_uint64 * 3)(), C.c_uint64(9), C.c_uint64(9)
    rows, cigar_offsets = (_lib.FmAlignment * 4)(), (C.c_uint64 * 5)()

    def seed(min_length=1, strands=3, max_occurrences=5, flags=0, reserved=0):
        return C.byref(_lib.FmSeedOptions(min_length, strands, max_occurrences, flags, reserved))

    def chain(max_gap=0, max_skew=0, gap_cost=1, min_score=1, max_matches=0, flags=0, reserved=0):
        return C.byref(_lib.FmChainOptions(max_gap, max_skew, gap_cost, min_score, max_matches, flags, reserved))

    def align(band=16, max_width=0, max_alignments=0, flags=0, reserved=0):
        return C.byref(_lib.FmAlignOptions(band, max_width, max_alignments, flags, reserved))

    def host(offs, bytes_, seed_opts, chain_opts, align_opts, out=out_offsets, total_rows=C.byref(n_rows), total_cigars=C.byref(n_cigars), rows_=None, cigar_offs=None):
        return L.gbwt_hip_fm_alignments(None, offs, bytes_, 2, seed_opts, chain_opts, align_opts, out, rows_, 4 if rows_ else 0, total_rows, cigar_offs, None, 0, total_cigars)

    # null outputs first
    assert host(offsets, data, seed(), chain(), align(), total_rows=None) == _lib.BAD_ARGUMENT and b"null totals" in L.gbwt_hip_last_error() and n_cigars.value == 0
    assert host(offsets, data, seed(), chain(), align(), total_cigars=None) == _lib.BAD_ARGUMENT and b"null totals" in L.gbwt_hip_last_error() and n_rows.value == 0
    assert host(offsets, data, seed(), chain(), align(), out=None) == _lib.BAD_ARGUMENT and b"null totals" in L.gbwt_hip_last_error()
    assert host(None, data, seed(strands=7), chain(flags=1), align(flags=1), rows_=rows) == _lib.BAD_ARGUMENT and b"null cigar offsets" in L.gbwt_hip_last_error()
    # then the reads
    assert host(None, data, seed(strands=7), chain(flags=1), align(flags=1)) == _lib.BAD_ARGUMENT and b"null pattern offsets" in L.gbwt_hip_last_error()
    assert host(descending, data, seed(strands=7), chain(flags=1), align(flags=1)) == _lib.BAD_ARGUMENT and b"do not ascend at pattern 1" in L.gbwt_hip_last_error()
    assert host(offsets, None, seed(strands=7), chain(flags=1), align(flags=1)) == _lib.BAD_ARGUMENT and b"null pattern bytes" in L.gbwt_hip_last_error()
    # then the seed options
    assert host(offsets, data, seed(strands=4), chain(flags=1), align(flags=1)) == _lib.BAD_ARGUMENT and b"strands" in L.gbwt_hip_last_error()
    assert host(offsets, data, seed(reserved=1), chain(flags=1), align(flags=1)) == _lib.BAD_ARGUMENT and b"flags and reserved of the seed options" in L.gbwt_hip_last_error()
    assert host(offsets, data, seed(max_occurrences=0), chain(flags=1), align(flags=1)) == _lib.BAD_ARGUMENT and b"chains need hits" in L.gbwt_hip_last_error()
    # then the chain options
    assert host(offsets, data, seed(), chain(flags=1), align(flags=1)) == _lib.BAD_ARGUMENT and b"flags and reserved of the chain options" in L.gbwt_hip_last_error()
    assert host(offsets, data, seed(), chain(max_gap=1 << 31), align(flags=1)) == _lib.BAD_ARGUMENT and b"at most 2^31 - 1" in L.gbwt_hip_last_error()
    assert host(offsets, data, seed(), chain(max_skew=1 << 16, gap_cost=1 << 15), align(band=5000)) == _lib.BAD_ARGUMENT and b"below 2^31" in L.gbwt_hip_last_error()
    # then the align options
    for bad in (dict(flags=1), dict(reserved=1), dict(max_width=1025), dict(band=1025), dict(band=1 << 31, max_width=3)):
        assert host(offsets, data, seed(), chain(), align(**bad)) == _lib.BAD_ARGUMENT and b"align options" in L.gbwt_hip_last_error(), bad
    # then the object
    for fine in (dict(), dict(band=0, max_width=1), dict(band=1024, max_width=1024, max_alignments=1 << 40)):
        assert host(offsets, data, seed(), chain(), align(**fine)) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error(), fine
    assert host(offsets, data, None, None, None) == _lib.BAD_ARGUMENT and b"chains need hits" in L.gbwt_hip_last_error()      # the default seed options ask for no hits
    assert host(offsets, data, seed(), None, None, rows_=rows, cigar_offs=cigar_offsets) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()
    assert (n_rows.value, n_cigars.value) == (0, 0)
    out = _lib.FmAlignmentRows()
    device = lambda *a: L.gbwt_hip_fm_alignments_device(None, *a)
    assert device(offsets, data, 2, 2, seed(), chain(), align(), None) == _lib.BAD_ARGUMENT and b"null output" in L.gbwt_hip_last_error()
    assert device(None, data, 2, 2, seed(), chain(), align(), C.byref(out)) == _lib.BAD_ARGUMENT and b"null pattern offsets" in L.gbwt_hip_last_error()
    assert device(offsets, data, 1 << 31, 2, seed(), chain(), align(), C.byref(out)) == _lib.BAD_ARGUMENT and b"too many patterns" in L.gbwt_hip_last_error()
    assert device(offsets, data, 2, 2, seed(), chain(flags=2), align(flags=2), C.byref(out)) == _lib.BAD_ARGUMENT and b"chain options" in L.gbwt_hip_last_error()
    assert device(offsets, data, 2, 2, seed(), chain(), align(max_width=2000), C.byref(out)) == _lib.BAD_ARGUMENT and b"align options" in L.gbwt_hip_last_error()
    assert device(offsets, data, 2, 2, seed(), chain(), align(), C.byref(out)) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()
    assert out.d_alignments is None and out.total_alignments == 0
    assert L.gbwt_hip_fm_last_align_info(None, C.byref(_lib.FmAlignInfo())) == _lib.BAD_ARGUMENT
    # the text calls: the object first
    assert L.gbwt_hip_fm_set_text(None, data, 2) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_set_text_device(None, data, 2, None) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_keep_path_text(None, None, None) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()


def test_python_align_arguments():
    assert api.ALIGNMENT_DTYPE.names == ("text_start", "text_end", "chain", "edit_distance", "width", "status", "strand", "path")
    opts = api.FMIndex._align_options(8, 128, 2)
    assert (opts.band, opts.max_width, opts.max_alignments, opts.flags, opts.reserved) == (8, 128, 2, 0, 0)
    for bad in ((-1, 0, 0), (1 << 32, 0, 0), (0, 1 << 32, 0), (0, 0, -1)):
        with pytest.raises(ValueError):
            api.FMIndex._align_options(*bad)
    assert api.cigar_string([(150 << 4) | 7]) == "150=" and api.cigar_string(np.array([(64 << 4) | 7, (2 << 4) | 1, (1 << 4) | 8, (3 << 4) | 2], dtype=np.uint32)) == "64=2I1X3D"
    assert api.cigar_string([]) == ""
    fm = api.FMIndex(None)                                                     # no object: the reads and the options are looked at first
    for bad, error in ((b"ACGT", TypeError), ([5], TypeError), ((np.array([0, 2, 1]), b"ACG"), ValueError)):
        with pytest.raises(error):
            fm.alignments(bad)
    with pytest.raises(ValueError):
        fm.alignments([b"ACGT"], strands=0)
    with pytest.raises(ValueError):
        fm.alignments([b"ACGT"], max_gap=-1)
    with pytest.raises(ValueError):
        fm.alignments([b"ACGT"], band=-1)
    with pytest.raises(ValueError):
        fm.alignments_device(0, 0, -1, 0)
    with pytest.raises(ValueError):
        fm.set_text(np.zeros((2, 2), dtype=np.uint8))
    import inspect
    assert inspect.signature(api.FMIndex.from_text).parameters["keep_text"].default is False and inspect.signature(api.GBZ.fm_index).parameters["keep_text"].default is False
    assert [inspect.signature(api.FMIndex.alignments).parameters[name].default for name in ("band", "max_width", "max_alignments")] == [16, 0, 0]
    assert hasattr(api.PathFMIndex, "keep_text")
