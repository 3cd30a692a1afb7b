"""GBWT construction without a GPU: the argument checks that answer before the device is touched, the checks of the Python mirror, and the
shared record encoder (csrc/build_codec.hpp) on the host against the oracle's ByteCode / RLE."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from gbwt_rs_amd import _lib
from test_merge_cpu import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-C", _lib.CSRC], stdout=subprocess.DEVNULL)


def message():
    return _lib.lib().gbwt_hip_last_error().decode()


def u64(values):
    return np.array(values, dtype=np.uint64)


def test_bad_path_sets_are_refused_before_the_device():
    L = _lib.lib()
    p = lambda a: a.ctypes.data
    offsets, nodes = u64([0, 2, 3]), u64([2, 5, 4])
    h = C.c_void_p(7)

    def build(off, nod, n, bidirectional=1, flags=_lib.OPEN_ALL, out=h):
        return L.gbwt_hip_build_from_paths(off, nod, n, bidirectional, 0, flags, C.byref(out) if out is not None else None)

    # null pointers
    assert build(p(offsets), p(nodes), 2, out=None) == _lib.BAD_ARGUMENT and "null output" in message()
    assert build(None, p(nodes), 2) == _lib.BAD_ARGUMENT and "null offsets" in message()
    assert h.value is None                                   # the output is cleared by a call that fails
    assert build(p(offsets), None, 2) == _lib.BAD_ARGUMENT and "null nodes" in message()
    # bidirectional is 0 or 1
    for b in (2, -1):
        assert build(p(offsets), p(nodes), 2, bidirectional=b) == _lib.BAD_ARGUMENT and "bidirectional" in message()
    # flags: a non-empty subset of the open flags
    for flags in (0, 8, 0x17):
        assert build(p(offsets), p(nodes), 2, flags=flags) == _lib.BAD_ARGUMENT and "flags" in message()
    # offsets: from 0, never decreasing
    assert build(p(u64([1, 2, 3])), p(nodes), 2) == _lib.BAD_ARGUMENT and "start at 0" in message()
    assert build(p(u64([0, 3, 2])), p(nodes), 2) == _lib.BAD_ARGUMENT and "decrease" in message() and "path 1" in message()
    # a node below 2: the endmarker and its flip are no nodes
    for bad in (0, 1):
        assert build(p(offsets), p(u64([2, bad, 4])), 2) == _lib.BAD_ARGUMENT and "below 2" in message() and "position 1" in message()
    # the same checks in front of the rows that are in HBM already (nothing is read through the pointers)
    rows = lambda off, nod, n, b=1, flags=_lib.OPEN_ALL, out=h: L.gbwt_hip_build_from_rows_device(off, nod, n, b, 0, flags, C.byref(out) if out is not None else None)
    assert rows(1 << 40, 1 << 40, 2, out=None) == _lib.BAD_ARGUMENT and "null output" in message()
    assert rows(None, 1 << 40, 2) == _lib.BAD_ARGUMENT and "null offsets" in message()
    assert rows(1 << 40, 1 << 40, 2, b=3) == _lib.BAD_ARGUMENT and "bidirectional" in message()
    assert rows(1 << 40, 1 << 40, 2, flags=0) == _lib.BAD_ARGUMENT and "flags" in message()


def test_sizes_beyond_32_bits_are_unsupported():
    """A node, a sequence count, or visits + sequences beyond 32 bits: the status and the wording of an open (gbwt_hip.h, "Widths")."""
    L = _lib.lib()
    p = lambda a: a.ctypes.data
    h = C.c_void_p()
    # a node that does not fit: alphabet_size would pass 2^32
    assert L.gbwt_hip_build_from_paths(p(u64([0, 2])), p(u64([2, 1 << 32])), 1, 1, 0, _lib.OPEN_ALL, C.byref(h)) == _lib.UNSUPPORTED
    assert "alphabet_size > 2^32 is not supported" in message()
    # visits + sequences (the nodes are never read: the sizes are refused in front of them)
    one = u64([2])
    for bidirectional, visits in ((0, (1 << 32) - 1), (1, 1 << 31), (0, 1 << 40)):
        assert L.gbwt_hip_build_from_paths(p(u64([0, visits])), p(one), 1, bidirectional, 0, _lib.OPEN_ALL, C.byref(h)) == _lib.UNSUPPORTED
        assert "2^32 - 1 are not supported" in message() and "sequences" in message()
    # an alphabet of 2^30 records or more
    assert L.gbwt_hip_build_from_paths(p(u64([0, 2])), p(u64([2, 1 << 31])), 1, 1, 0, _lib.OPEN_ALL, C.byref(h)) == _lib.UNSUPPORTED
    assert "2^30 records" in message()


def test_records_save_and_info_want_a_handle():
    L = _lib.lib()
    n, m = C.c_uint64(5), C.c_uint64(5)
    assert L.gbwt_hip_records(None, None, 0, C.byref(n), None, 0, C.byref(m)) == _lib.BAD_ARGUMENT and "null" in message()
    assert (n.value, m.value) == (0, 0)
    assert L.gbwt_hip_save(None, b"/nonexistent/x.gbwt") == _lib.BAD_ARGUMENT
    info = _lib.BuildInfo()
    assert L.gbwt_hip_last_build_info(None, C.byref(info)) == _lib.BAD_ARGUMENT
    assert C.sizeof(_lib.BuildInfo) == 72


def test_python_mirror_validates_before_it_calls(monkeypatch):
    import gbwt_rs_amd as G

    def never(*args):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib.lib(), "gbwt_hip_build_from_paths", never)
    monkeypatch.setattr(_lib.lib(), "gbwt_hip_build_from_rows_device", never)
    with pytest.raises(ValueError):
        G.GBWT.from_paths([np.zeros((2, 2), dtype=np.uint64)])            # two-dimensional
    with pytest.raises(ValueError):
        G.GBWT.from_paths([[2, 4], [[2], [4]]])
    with pytest.raises(ValueError):
        G.GBWT.from_paths([[2, -4, 6]])                                    # negative
    with pytest.raises(ValueError):
        G.GBWT.from_paths([np.array([2, 4]), np.array([-1], dtype=np.int64)])
    with pytest.raises(TypeError):
        G.GBWT.from_paths([[2.5, 4.0]])
    with pytest.raises(TypeError):
        G.GBWT.from_rows_device(np.zeros(3, dtype=np.uint64), 1)
    with pytest.raises(ValueError):
        G.GBWT.from_rows_device(_lib.Paths(), 1)                           # more rows than the struct holds
    for method in ("from_paths", "from_rows_device", "records", "save", "last_build_info"):
        assert callable(getattr(G.GBWT, method)), method


def test_build_codec_against_the_oracle(tmp_path):
    """tests/cpp/build_codec.cpp: build_codec.hpp's size and write functions on the host under ASan + UBSan; the bytes against the oracle's
    ByteCode (src/support.rs:1063-1070) and RLE (src/support.rs:1238-1248) encoders, the sizes against the lengths of those bytes."""
    exe = tmp_path / "build_codec"
    subprocess.run([host_compiler(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", _lib.CSRC,
                    os.path.join(ROOT, "tests", "cpp", "build_codec.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "done"
    seen = {"varint": set(), "run": set(), "header": 0, "edge": 0}
    for line in lines[:-1]:
        kind, *fields = line.split()
        size, got = int(fields[-2]), bytes.fromhex(fields[-1])
        args = [int(x) for x in fields[:-2]]
        if kind == "varint" or kind == "header":
            want = O.bytecode_encode(args)
        elif kind == "edge":
            want = O.bytecode_encode(args)                   # delta, then offset
        else:
            assert kind == "run", line
            sigma, value, length = args
            want = O.rle_encode(sigma, [(value, length)])
        assert got == want, (line, want.hex())
        assert size == len(want), line
        if kind == "varint":
            seen["varint"].add(args[0])
        elif kind == "run":
            seen["run"].add((args[0], args[2]))
        else:
            seen[kind] += 1
    assert seen["varint"] == {0, 127, 128, 16383, 16384, 2**32 - 1}
    for sigma in (1, 2, 85, 86, 128, 129, 254, 255, 300):
        threshold = 256 // sigma
        lens = {n for n in (1, threshold - 1, threshold, threshold + 127, threshold + 128, 100000) if n >= 1}
        assert {n for s, n in seen["run"] if s == sigma} == lens, sigma
    assert seen["header"] == 6 and seen["edge"] == 36


def test_build_kernels_compile_without_scratch():
    """Every kernel of build.hip for gfx950: nothing spilled, no scratch."""
    import re
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                          os.path.join(_lib.CSRC, "build.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = set()
    for at, line in enumerate(lines):
        if "Function Name" in line and "k_build_" in line:
            block = "\n".join(lines[at:at + 14])
            assert int(re.search(r"VGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"SGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)) == 0, block
            seen.add(re.search(r"(k_build_[a-z_]+?)E", line).group(1))
    for kernel in ("k_build_expand", "k_build_round_keys", "k_build_gather", "k_build_edge_offsets", "k_build_run_sizes", "k_build_fill_edges", "k_build_fill_runs"):
        assert kernel in seen, (kernel, sorted(seen))
