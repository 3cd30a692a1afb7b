"""GBZ::reference_positions without a GPU: the C ABI declares, exports and types the entry points, the kernels compile for gfx950 without
scratch, and the yardstick of tests/test_gpu_refpos.py (tests/refpos_expect.py) is pinned on the golden graphs the way the reference pins
its own (src/gbz/tests.rs:521-567): against the full list of node starts of an oracle walk, for interval 0 .. 9."""
import os
import re
import subprocess

import numpy as np

import oracle_lib as O
import refpos_expect as R
from gbwt_rs_amd import _lib

NEW_SYMBOLS = ["gbwt_hip_reference_sample_names", "gbwt_hip_reference_paths", "gbwt_hip_path_positions_device", "gbwt_hip_path_positions",
               "gbwt_hip_reference_positions", "gbwt_hip_last_positions_ms", "gbwt_hip_last_positions_rounds"]


def test_entry_points_declared_exported_and_typed():
    header = open(_lib.HEADER).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"gbwt_hip_status\s+" + name + r"\(", header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    from test_capi_cpu import declared_symbols
    assert set(declared_symbols()) == set(_lib.SIGNATURES)                     # what test_header_symbols_exported keeps comparing
    import ctypes as C
    assert C.sizeof(_lib.ReferencePath) == 32 and C.sizeof(_lib.ReferencePosition) == 24
    from gbwt_rs_amd import GBZ, api
    assert api.REFPATH_DTYPE.itemsize == 32 and api.REFPOS_DTYPE.itemsize == 24
    for method in ("reference_sample_names", "reference_paths", "path_positions", "path_positions_device", "reference_positions", "last_positions_ms"):
        assert callable(getattr(GBZ, method)), method


def test_refpos_kernels_compile_without_scratch():
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                          os.path.join(_lib.CSRC, "refpos.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = {}
    for at, line in enumerate(lines):
        if "Function Name" in line and "k_refpos" in line:
            block = "\n".join(lines[at:at + 14])
            assert int(re.search(r"VGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"SGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)) == 0, block
            seen[line.split("Function Name: ")[1].split()[0]] = int(re.search(r"VGPRs: (\d+)", block).group(1))
    assert len([name for name in seen if "k_refpos_walk" in name]) == 2, seen  # the O(1) step and the step on the record bytes
    for kernel in ("k_refpos_lengths", "k_refpos_succ", "k_refpos_round", "k_refpos_paths"):
        assert any(kernel in name for name in seen), (kernel, seen)


def test_reference_sample_rule():
    names = ["s0", "s1", "s2", "_gbwt_ref"]
    assert R.reference_sample_names(names, None, True) == ["_gbwt_ref"] and R.reference_sample_names(names, None, False) == []
    assert R.reference_sample_names(names, "s2 nosuch s0", True) == ["s2", "s0", "_gbwt_ref"]
    assert R.reference_sample_names(names, "s2  s0", False) == ["s2", "s0"]    # (the empty piece between two blanks names no sample)
    assert R.reference_sample_names(["s0"], "s0", True) == ["s0"]              # no generic sample in the dictionary
    samples = [3, 0, 1, 2, 0, 3, 1]
    assert R.reference_paths(names, samples, "s0 nosuch", True) == [0, 1, 4, 5]
    assert R.reference_paths(names, samples, "s0 nosuch", False) == [1, 4]
    assert R.reference_paths(names, samples, "nosuch", False) == []
    assert R.kept(np.array([0, 1, 2, 3], dtype=np.uint64), 0).tolist() == [0, 1, 2, 3]
    assert R.kept(np.array([0, 3, 4, 6, 7], dtype=np.uint64), 3).tolist() == [0, 1, 3]        # 3 >= 0 + 3 and 6 >= 3 + 3: `>=`
    assert R.kept(np.array([0, 5, 2 ** 63], dtype=np.uint64), 2 ** 64 - 1).tolist() == [0]
    assert R.kept(np.zeros(0, dtype=np.uint64), 7).tolist() == []


def check_like_the_reference(gbwt, ref_paths, lengths):
    """src/gbz/tests.rs:528-566 with the helper in the place of GBZ::reference_positions."""
    starts = {p: R.node_starts(gbwt, p, lengths) for p in ref_paths}
    for p in ref_paths:                                                        # the walk is the oracle's sequence
        assert starts[p][2][:, 0].tolist() == gbwt.sequence(2 * p)
    for interval in range(10):
        paths = [R.positions_of(starts[p], p, interval) for p in ref_paths]
        assert len(paths) == len(ref_paths)
        for (pid, length, offsets, positions), p in zip(paths, ref_paths):
            assert pid == p and length == starts[p][0]
            nxt, at = 0, 0
            for offset, pos in zip(starts[p][1].tolist(), starts[p][2].tolist()):
                if offset >= nxt:
                    assert at < offsets.size, (p, interval)
                    assert int(offsets[at]) == offset and positions[at].tolist() == pos, (p, interval)
                    at += 1
                    nxt = offset + interval
            assert at == offsets.size, (p, interval)
    return starts


def test_example_like_the_reference():
    gbwt = O.OracleGBZ(os.path.join(O.GOLDEN, "example.gbz")).gbwt()
    lengths, samples, path_samples = R.golden("example.gbz")
    assert samples == ["_gbwt_ref", "sample"] and path_samples == [0, 0, 1, 1, 1, 1]
    ref_paths = R.reference_paths(samples, path_samples, None)
    assert ref_paths == [0, 1]                                                 # P-lines A and B
    starts = check_like_the_reference(gbwt, ref_paths, lengths)
    assert starts[0][0] == 5 and starts[1][0] == 4
    assert R.positions_of(starts[0], 0, 2)[2].tolist() == [0, 2, 4] and R.positions_of(starts[1], 1, 2)[2].tolist() == [0, 2]
    assert starts[0][2][:, 0].tolist() == [22, 24, 28, 30, 34] and starts[1][2][:, 0].tolist() == [42, 44, 48, 50]
    assert starts[0][2][0].tolist() == list(gbwt.start(0))
    # every path of the file, not only the reference ones: the reverse visits of W-line >21>22>24<23<21
    every = check_like_the_reference(gbwt, list(range(6)), lengths)
    assert [every[p][0] for p in range(6)] == [5, 4, 5, 5, 5, 4]
    assert every[4][2][:, 0].tolist() == [42, 44, 48, 47, 43]


def test_translation_like_the_reference():
    lengths, samples, path_samples = R.golden("translation.gbz")
    assert path_samples == [0, 1, 1] and lengths.tolist() == [0, 2, 1, 1, 1, 2, 1, 2, 1, 1, 1, 2]
    gbwt = O.OracleGBZ(os.path.join(O.GOLDEN, "translation.gbz")).gbwt()
    ref_paths = R.reference_paths(samples, path_samples, None)
    assert ref_paths == [0]
    starts = check_like_the_reference(gbwt, [0, 1, 2], lengths)
    assert [starts[p][0] for p in range(3)] == [10, 10, 10]                    # the end coordinates of the W-lines
    assert starts[0][1].tolist() == [0, 2, 3, 4, 6, 7, 8] and R.positions_of(starts[0], 0, 3)[2].tolist() == [0, 3, 6]
