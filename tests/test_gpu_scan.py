"""The prefix sums of the library (csrc/scan.hpp) on the GPU itself, without an index: tests/cpp/scan_device_check.hip, built with csrc/scan.hip,
runs launch_scan in pieces of 1 024 and 4 096 items and in one piece over n = 0, 1, piece - 1, piece, piece + 1, 2 piece, 2 piece + 1 and
3 piece + 17 items below 2^40 -- the smallest shapes at which a piece boundary, a last partial piece and an empty scan can each go wrong --
and launch_block_scan over 1 and 1 025 items, against host prefix sums: exact sums, out[0] == 0, the input unchanged, the word behind the
output untouched, with temp storage of exactly scan_temp_bytes(n, piece)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

PIECES = [1024, 4096, 1 << 30]


def sizes(piece):
    p = 4096 if piece == 1 << 30 else piece
    return [0, 1, p - 1, p, p + 1, 2 * p, 2 * p + 1, 3 * p + 17]


def test_scans_on_the_device(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "gbwt_rs_amd", "csrc")
    exe = tmp_path / "scan_device_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", csrc, os.path.join(root, "tests", "cpp", "scan_device_check.hip"),
                    os.path.join(csrc, "scan.hip"), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    for piece in PIECES:
        for n in sizes(piece):
            assert f"ok scan n={n} piece={piece}" in lines, (n, piece)
    for n in (1, 1025):
        assert f"ok block_scan n={n}" in lines, n
    assert lines[-1] == "done" and len(lines) == 8 * len(PIECES) + 2 + 1
