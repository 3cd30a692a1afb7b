"""The chains of seeds without a GPU: the yardstick of tests/chain_expect.py against its own slow definition and the conditions of a
peeling, the shared arithmetic (csrc/fm_chains.hpp) and the host-side plan (csrc/fm_chain_plan.hpp) as programs of their own under ASan +
UBSan, the resources of the kernels of csrc/fm_chains.hip, and the argument checks of the C ABI that answer before a device is touched."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import chain_expect as X
import fm_expect as F
import sa_expect as A
import seed_expect as E
from gbwt_rs_amd import _lib, api
from test_merge_cpu import sanitized_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [(1000, 50, 1, 1), (1000, 2, 1, 1), (100, 10, 2, 20), (1000, 150, 0, 1)]


def replaced(read, at=(40, 90)):
    """`read` with the bases at `at` replaced by the next one of ACGT."""
    r = bytearray(read)
    for k in at:
        r[k] = b"ACGT"[(b"ACGT".index(r[k]) + 1) % 4]
    return bytes(r)


def case_reads(text):
    """The reads of the first case: a cut, two bases replaced, 3 deleted, 5 inserted, two pieces, a reverse complement, and empties."""
    long = text[30:180]
    return [text[10:160], replaced(text[20:170]), long[:70] + long[73:], long[:70] + b"ACGTA" + long[70:], text[5:60] + text[200:260],
            E.reverse_complement(replaced(text[20:170])), b"", b"A", b"ZZZ"]


@functools.lru_cache(maxsize=None)
def case_text():
    text = A.mutated_rows(4, 300, 3)
    return text, F.suffix_array(text)


def items_of(text, sa, reads, min_length=5):
    for read in reads:
        for strand in (E.FORWARD, E.REVERSE):
            matches = X.matches_of(text, sa, read, strand, min_length)
            y, x, w = ([m[k] for m in matches] for k in range(3))
            yield y, x, w


def test_dp_is_the_slow_definition_and_peeling_partitions():
    text, sa = case_text()
    periodic = b"AC" * 40 + b"\0"
    inputs = [(text, sa, case_reads(text), None), (text, sa, case_reads(text), [0, 301, 602, 903, 1204]),
              (periodic, F.suffix_array(periodic), [b"ACACAC" + b"G" + b"ACACAC"], None)]
    seen_pred = seen_tie = seen_no_gain = False
    for t, s, reads, bounds in inputs:
        for y, x, w in items_of(t, s, reads):
            seg = X.segments(y, bounds)
            for setting in SETTINGS + [(400, 8, 1, 1)]:
                opts = X.options(*setting)
                f, pred, pairs = X.dp(y, x, w, seg, opts)
                assert (f, pred, pairs) == X.dp_slow(y, x, w, seg.tolist(), opts)
                chains = X.peel(f, pred)
                members = [k for _, _, row in chains for k in row]
                assert sorted(members) == list(range(len(y)))                        # every match is in exactly one chain of the peeling
                assert all(row == sorted(row) for _, _, row in chains)
                if chains:                                                           # the first chain is the best: the maximal f, base 0
                    assert chains[0][0] == max(f) and chains[0][1] == 0
                    seen_no_gain |= any(score < 1 for score, _, _ in chains)      # behind a used predecessor: never reported
                seen_pred |= any(p != X.NONE for p in pred)
                for i, p in enumerate(pred):                                         # a tie: another admissible j gives the same score
                    if p == X.NONE:
                        continue
                    for j in range(p):
                        dy, dx = y[i] - y[j], x[i] - x[j]
                        if seg[j] == seg[i] and 1 <= dy <= opts[0] and 1 <= dx <= opts[0] and abs(dy - dx) <= opts[1]:
                            seen_tie |= f[j] + min(w[i], dx, dy) - opts[2] * abs(dy - dx) == f[i]
    assert seen_pred and seen_tie and seen_no_gain


def best_forward(out, k):
    rows = [row for row in out["chains"][out["read_offsets"][k]:out["read_offsets"][k + 1]] if row[6] == E.FORWARD]
    return rows[0] if rows else None


def test_known_chains_of_the_first_case():
    """The figures the definition gives for the reads of the first case: the device tests compare against the same yardstick."""
    text, sa = case_text()
    reads = case_reads(text)
    out = X.expected_rows(text, sa, reads, 5, E.BOTH, 1 << 20, 1000, 50, 1, 1)
    assert out["items"] == 18 and out["read_offsets"][-1] == len(out["chains"]) == len(out["match_offsets"]) - 1
    assert best_forward(out, 0)[4:6] == (150, 1)
    assert best_forward(out, 1)[4:6] == (131, 3)                                 # two bases replaced: three matches
    assert best_forward(out, 2)[4:6] == (137, 2)                                 # 3 bases deleted: 70 + min(77, 70, 73) - 3
    assert best_forward(out, 3)[4:6] == (135, 2)                                 # 5 bases inserted: 70 + min(75, 75, 70) - 5
    # the two pieces lie 195 apart in the text and 55 in the read: skew 140
    joined = lambda o: [row for row in o["chains"][o["read_offsets"][4]:o["read_offsets"][5]] if row[6] == E.FORWARD and row[5] >= 2 and row[2] < 40 and row[3] > 80]
    assert not joined(out)
    free = X.expected_rows(text, sa, reads, 5, E.BOTH, 1 << 20, 1000, 150, 0, 1)
    assert joined(free) and joined(free)[0][4:6] == (108, 2)                    # the second piece matches from 53 on: 55 + min(62, 53, 193)
    assert not joined(X.expected_rows(text, sa, reads, 5, E.BOTH, 1 << 20, 1000, 139, 0, 1))
    # the reverse complement of the replaced read chains on the reverse strand as the read itself does on the forward strand
    reverse = [row for row in out["chains"][out["read_offsets"][5]:out["read_offsets"][6]] if row[6] == E.REVERSE]
    assert reverse[0][:6] == best_forward(out, 1)[:6]
    assert out["read_offsets"][6:] == [out["read_offsets"][6]] * 4               # the empty read, A and ZZZ: no seed of 5 bytes
    # items with more than one chain, and skew rejections: a tighter skew admits fewer pairs
    assert any(out["read_offsets"][k + 1] - out["read_offsets"][k] > 2 for k in range(6))
    tight = X.expected_rows(text, sa, reads, 5, E.BOTH, 1 << 20, 1000, 2, 1, 1)
    assert 0 < tight["pairs"] < out["pairs"] and tight["n_matches"] == out["n_matches"]
    # identical rows: four equal chains in ascending index order, then single matches
    same = A.mutated_rows(4, 300, 0)
    equal = X.expected_rows(same, F.suffix_array(same), [replaced(same[20:170])], 5, E.FORWARD, 1 << 20, 1000, 50, 1, 1)
    assert [row[4:6] for row in equal["chains"][:4]] == [(131, 3)] * 4 and [row[0] for row in equal["chains"][:4]] == [20, 321, 622, 923]
    assert all(row[5] == 1 for row in equal["chains"][4:])
    # segments: the end of one row and the start of the next join on a plain text and must not with bounds
    across = [text[240:300] + text[301:341]]
    plain = X.expected_rows(text, sa, across, 5, E.FORWARD, 1 << 20, 1000, 50, 1, 1)
    cut = X.expected_rows(text, sa, across, 5, E.FORWARD, 1 << 20, 1000, 50, 1, 1, bounds=[0, 301, 602, 903, 1204])
    assert plain["chains"][0][4:6] == (99, 2) and cut["chains"][0][4:6] == (60, 1) and {row[7] for row in cut["chains"]} <= {0, 1, 2, 3}
    # max_matches: an item above it is skipped and counted
    few = X.expected_rows(text, sa, reads[1:2], 5, E.FORWARD, 1 << 20, 1000, 50, 1, 1, max_matches=2)
    assert few["skipped_items"] == 1 and few["chains"] == [] and few["n_matches"] == 0
    assert X.expected_rows(text, sa, reads[1:2], 5, E.FORWARD, 1 << 20, 1000, 50, 1, 1, max_matches=3)["chains"] == out["chains"][out["read_offsets"][1]:][:1]


CHAIN_CASES = ("ties", "ties_free", "ties_cut", "signed", "scattered", "segments", "defaults", "high", "empty")
PLAN_CASES = ("constants", "nothing", "item_bytes", "hit_bytes", "temp_and_words", "scratch_is_the_sum", "few_hits", "capacity_exact_fit", "capacity_one_byte_short",
              "hits_refused_before_memory", "most_hits")


def test_chain_arithmetic_under_sanitizers(tmp_path):
    """tests/cpp/fm_chains.cpp: the DP and the peeling with the functions of fm_chains.hpp over host arrays -- equal-score ties, a signed c,
    windows cut by the gap and by segments, y at the top of the range -- against the yardstick over the inputs the program prints."""
    got, lines = sanitized_program(tmp_path, "fm_chains")
    numbers = lambda key: [int(v) for v in got.get(key, "").split()]
    assert [line.split(".")[0] for line in lines if ".options" in line] == list(CHAIN_CASES)
    for case in CHAIN_CASES:
        opts = X.options(*numbers(case + ".options"))
        y, x, w, seg = (numbers(f"{case}.{name}") for name in "y x w seg".split())
        assert len(y) == len(x) == len(w) == len(seg) and sorted(zip(y, x)) == list(zip(y, x)) and (case == "empty") == (not y)
        f, pred, pairs = X.dp_slow(y, x, w, seg, opts)
        assert numbers(case + ".f") == f and numbers(case + ".pred") == pred and numbers(case + ".pairs") == [pairs], case
        want = []
        for score, _, members in X.peel(f, pred):
            if score >= opts[3]:
                first, last = members[0], members[-1]
                summary = (y[first], y[last] + w[last], x[first], x[last] + w[last], score, len(members), 1, seg[last])
                want.append(",".join(map(str, summary)) + ":" + "+".join(map(str, members)))
        assert got.get(case + ".chains", "").split() == want, case
        if case.startswith("ties"):                                              # dy 6 and dy 8 give the same score: the larger j wins
            assert len(set(f)) < len(f) and any(p != X.NONE for p in pred)
    assert min(numbers("signed.f")) >= 4 and numbers("signed.pairs")[0] > 0
    assert max(numbers("high.y")) + 25 > 1 << 32 and numbers("high.pairs")[0] > 0


def test_chain_plan_under_sanitizers(tmp_path):
    """tests/cpp/fm_chain_plan.cpp: the bytes of the scratch against hand-computed sizes, an exact fit, one byte short, and the refusal."""
    _, lines = sanitized_program(tmp_path, "fm_chain_plan")
    assert lines == ["ok " + case for case in PLAN_CASES] + ["done"]


def test_chain_kernels_compile_without_scratch():
    """Every kernel of fm_chains.hip for gfx950: nothing spilled, no scratch; the DP within 64 VGPRs and 24 KB of LDS a workgroup."""
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                          os.path.join(_lib.CSRC, "fm_chains.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = {}
    for at, line in enumerate(lines):
        if "Function Name" in line and "k_chain_" in line:
            block = "\n".join(lines[at:at + 14])
            assert int(re.search(r"VGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"SGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)) == 0, block
            seen[re.search(r"\d+(k_chain_[a-z_]+?)E", line).group(1)] = (int(re.search(r" VGPRs: (\d+)", block).group(1)), int(re.search(r"LDS Size \[bytes/block\]: (\d+)", block).group(1)))
    assert sorted(seen) == ["k_chain_dp", "k_chain_expand", "k_chain_fill", "k_chain_item_counts", "k_chain_peel", "k_chain_unpack", "k_chain_visit_keys"], sorted(seen)
    assert seen["k_chain_dp"][0] <= 64 and seen["k_chain_dp"][1] == 4 * 512 * 12, seen


def test_chain_symbols_in_the_header_and_the_library():
    header = open(os.path.join(ROOT, "include", "gbwt_hip.h")).read()
    L = _lib.lib()
    for name in ("gbwt_hip_fm_chains", "gbwt_hip_fm_chains_device", "gbwt_hip_fm_last_chain_info"):
        assert re.search(r"gbwt_hip_status " + name + r"\(", header) and getattr(L, name)
    for name in ("gbwt_hip_fm_chain_options", "gbwt_hip_fm_chain", "gbwt_hip_fm_chain_match", "gbwt_hip_fm_chain_info", "gbwt_hip_fm_chain_rows"):
        assert re.search(r"\} " + name + r";", header), name
    assert C.sizeof(_lib.FmChain) == 40 == api.CHAIN_DTYPE.itemsize and C.sizeof(_lib.FmChainMatch) == 16 == api.CHAIN_MATCH_DTYPE.itemsize and C.sizeof(_lib.FmChainOptions) == 32
    for struct, dtype in ((_lib.FmChain, api.CHAIN_DTYPE), (_lib.FmChainMatch, api.CHAIN_MATCH_DTYPE)):
        assert [dtype.fields[name][1] for name, _ in struct._fields_] == [getattr(struct, name).offset for name, _ in struct._fields_]
        assert dtype.names == tuple(name for name, _ in struct._fields_)


def test_chain_argument_checks_answer_before_the_device():
    L = _lib.lib()
    offsets, descending = (C.c_uint64 * 3)(0, 1, 2), (C.c_uint64 * 3)(0, 2, 1)
    data, out_offsets, n_chains, n_matches = (C.c_uint8 * 2)(65, 67), (C.c_uint64 * 3)(), C.c_uint64(9), C.c_uint64(9)
    chains, match_offsets = (_lib.FmChain * 4)(), (C.c_uint64 * 5)()

    def seed(min_length=1, strands=3, max_occurrences=5, flags=0, reserved=0):
        return C.byref(_lib.FmSeedOptions(min_length, strands, max_occurrences, flags, reserved))

    def chain(max_gap=0, max_skew=0, gap_cost=1, min_score=1, max_matches=0, flags=0, reserved=0):
        return C.byref(_lib.FmChainOptions(max_gap, max_skew, gap_cost, min_score, max_matches, flags, reserved))

    def host(offs, bytes_, seed_opts, chain_opts, out=out_offsets, total_chains=C.byref(n_chains), total_matches=C.byref(n_matches), chains_=None, match_offs=None):
        return L.gbwt_hip_fm_chains(None, offs, bytes_, 2, seed_opts, chain_opts, out, chains_, 4 if chains_ else 0, total_chains, match_offs, None, 0, total_matches)

    # null outputs first
    assert host(offsets, data, seed(), chain(), total_chains=None) == _lib.BAD_ARGUMENT and b"null totals" in L.gbwt_hip_last_error() and n_matches.value == 0
    assert host(offsets, data, seed(), chain(), total_matches=None) == _lib.BAD_ARGUMENT and b"null totals" in L.gbwt_hip_last_error() and n_chains.value == 0
    assert host(offsets, data, seed(), chain(), out=None) == _lib.BAD_ARGUMENT and b"null totals" in L.gbwt_hip_last_error()
    assert host(None, data, seed(strands=7), chain(flags=1), chains_=chains) == _lib.BAD_ARGUMENT and b"null match offsets" in L.gbwt_hip_last_error()
    # then the reads
    assert host(None, data, seed(strands=7), chain(flags=1)) == _lib.BAD_ARGUMENT and b"null pattern offsets" in L.gbwt_hip_last_error()
    assert host(descending, data, seed(strands=7), chain(flags=1)) == _lib.BAD_ARGUMENT and b"do not ascend at pattern 1" in L.gbwt_hip_last_error()
    assert host(offsets, None, seed(strands=7), chain(flags=1)) == _lib.BAD_ARGUMENT and b"null pattern bytes" in L.gbwt_hip_last_error()
    # then the seed options, as the seeds call checks them, and that hits are asked for
    for strands in (0, 4):
        assert host(offsets, data, seed(strands=strands, flags=1), chain(flags=1)) == _lib.BAD_ARGUMENT and b"strands" in L.gbwt_hip_last_error()
    assert host(offsets, data, seed(flags=1, max_occurrences=0), chain(flags=1)) == _lib.BAD_ARGUMENT and b"flags and reserved of the seed options" in L.gbwt_hip_last_error()
    assert host(offsets, data, seed(reserved=1), chain(flags=1)) == _lib.BAD_ARGUMENT and b"flags and reserved of the seed options" in L.gbwt_hip_last_error()
    assert host(offsets, data, seed(max_occurrences=0), chain(flags=1)) == _lib.BAD_ARGUMENT and b"chains need hits" in L.gbwt_hip_last_error()
    assert host(offsets, data, None, chain(flags=1)) == _lib.BAD_ARGUMENT and b"chains need hits" in L.gbwt_hip_last_error()
    # then the chain options
    assert host(offsets, data, seed(), chain(flags=1, max_gap=1 << 31)) == _lib.BAD_ARGUMENT and b"flags and reserved of the chain options" in L.gbwt_hip_last_error()
    assert host(offsets, data, seed(), chain(reserved=1)) == _lib.BAD_ARGUMENT and b"flags and reserved of the chain options" in L.gbwt_hip_last_error()
    for wide in (dict(max_gap=1 << 31), dict(max_skew=1 << 31)):
        assert host(offsets, data, seed(), chain(gap_cost=1 << 31, **wide)) == _lib.BAD_ARGUMENT and b"at most 2^31 - 1" in L.gbwt_hip_last_error()
    assert host(offsets, data, seed(), chain(max_skew=1 << 16, gap_cost=1 << 15)) == _lib.BAD_ARGUMENT and b"below 2^31" in L.gbwt_hip_last_error()
    assert host(offsets, data, seed(), chain(gap_cost=4294968)) == _lib.BAD_ARGUMENT and b"below 2^31" in L.gbwt_hip_last_error()      # x the 500 that 0 stands for
    # then the object
    assert host(offsets, data, seed(), chain(max_skew=(1 << 31) - 1, max_gap=(1 << 31) - 1, gap_cost=1)) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()
    assert host(offsets, data, seed(), chain(gap_cost=4294967)) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()
    assert host(offsets, data, seed(), None, chains_=chains, match_offs=match_offsets) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()
    assert (n_chains.value, n_matches.value) == (0, 0)
    rows = _lib.FmChainRows()
    assert L.gbwt_hip_fm_chains_device(None, offsets, data, 2, 2, seed(), chain(), None) == _lib.BAD_ARGUMENT and b"null output" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_chains_device(None, None, data, 2, 2, seed(), chain(), C.byref(rows)) == _lib.BAD_ARGUMENT and b"null pattern offsets" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_chains_device(None, offsets, data, 1 << 31, 2, seed(), chain(), C.byref(rows)) == _lib.BAD_ARGUMENT and b"too many patterns" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_chains_device(None, offsets, data, 2, 2, seed(max_occurrences=0), chain(), C.byref(rows)) == _lib.BAD_ARGUMENT and b"chains need hits" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_chains_device(None, offsets, data, 2, 2, seed(), chain(flags=2), C.byref(rows)) == _lib.BAD_ARGUMENT and b"chain options" in L.gbwt_hip_last_error()
    assert L.gbwt_hip_fm_chains_device(None, offsets, data, 2, 2, seed(), chain(), C.byref(rows)) == _lib.BAD_ARGUMENT and b"null FM-index" in L.gbwt_hip_last_error()
    assert rows.d_chains is None and rows.total_chains == 0
    assert L.gbwt_hip_fm_last_chain_info(None, C.byref(_lib.FmChainInfo())) == _lib.BAD_ARGUMENT


def test_python_chain_arguments():
    assert api.CHAIN_DTYPE.names == ("text_start", "text_end", "read_start", "read_end", "score", "matches", "strand", "path") and api.CHAIN_MATCH_DTYPE.names == ("y", "x", "w")
    opts = api.FMIndex._chain_options(1000, 50, 2, 20, 7)
    assert (opts.max_gap, opts.max_skew, opts.gap_cost, opts.min_score, opts.max_matches, opts.flags, opts.reserved) == (1000, 50, 2, 20, 7, 0, 0)
    for bad in ((-1, 0, 1, 1, 0), (0, 1 << 32, 1, 1, 0), (0, 0, -1, 1, 0), (0, 0, 1, 1, -1)):
        with pytest.raises(ValueError):
            api.FMIndex._chain_options(*bad)
    fm = api.FMIndex(None)                                                     # no object: the reads and the options are looked at first
    for bad, error in ((b"ACGT", TypeError), ([5], TypeError), ((np.array([0, 2, 1]), b"ACG"), ValueError)):
        with pytest.raises(error):
            fm.chains(bad)
    with pytest.raises(ValueError):
        fm.chains([b"ACGT"], strands=0)
    with pytest.raises(ValueError):
        fm.chains([b"ACGT"], max_gap=-1)
    with pytest.raises(ValueError):
        fm.chains_device(0, 0, -1, 0)
