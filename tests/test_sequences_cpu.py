"""The bases of GBZ paths without a GPU: the C ABI declares, exports and types the entry points, the bases kernels compile for gfx950
without spills, and the numpy expected-value helper of tests/test_gpu_sequences.py agrees with the golden GFA."""
import os
import re
import subprocess

import numpy as np

from gbwt_rs_amd import _lib
import seq_expect as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_SYMBOLS = ["gbwt_hip_path_sequences_device", "gbwt_hip_path_sequences", "gbwt_hip_node_sequence", "gbwt_hip_write_sequences",
               "gbwt_hip_last_sequences_ms"]


def test_entry_points_declared_exported_and_typed():
    header = open(_lib.HEADER).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"gbwt_hip_status\s+" + name + r"\(", header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_bases_kernels_compile_without_spills():
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                          os.path.join(_lib.CSRC, "sequences.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = 0
    for at, line in enumerate(lines):
        if "Function Name" in line and ("k_bases" in line or "k_chunk_bases" in line):
            block = "\n".join(lines[at:at + 14])
            assert int(re.search(r"VGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)) == 0, block
            seen += 1
    assert seen == 2


def test_complement_table():
    c = E.COMPLEMENT
    assert bytes(c[list(b"ACGTacgt")]) == b"TGCATGCA"
    assert bytes(c[list(b"NnRYKMSWBDHV-*\x00\xff")]) == b"N" * 16


def test_expected_values_against_example_gfa():
    gfa = open(os.path.join(GOLDEN, "example.gfa"), "rb").read()
    table = E.LabelTable.from_gfa(gfa)
    labels = E.s_lines(gfa)
    # P-line A: 11+,12+,14+,15+,17+ (tests/golden/example.gfa)
    p_line = next(l for l in gfa.split(b"\n") if l.startswith(b"P\tA\t"))
    steps = p_line.split(b"\t")[2].split(b",")
    ids = [int(s[:-1]) for s in steps]
    rev = [s.endswith(b"-") for s in steps]
    offsets, data = E.expected_rows(table, [(ids, rev)], endmarker=0)
    assert data == b"".join(labels[str(i).encode()] for i in ids) + b"\x00"
    assert offsets.tolist() == [0, len(data)]
    # the reverse orientation of the same path: the nodes backwards, each reverse-complemented
    _, back = E.expected_rows(table, [(ids[::-1], [not r for r in rev][::-1])])
    fwd = np.frombuffer(data[:-1], dtype=np.uint8)
    assert back == E.COMPLEMENT[fwd[::-1]].tobytes()
    # a missing path is an empty row without endmarker; an empty path is the endmarker alone
    offsets, data = E.expected_rows(table, [None, ([], []), ([11], [True])], endmarker=7)
    assert offsets.tolist() == [0, 0, 1, 3] and data == b"\x07" + E.COMPLEMENT[list(labels[b"11"])].tobytes() + b"\x07"
