"""Construction from GFA without a GPU: the argument checks that answer before the device is touched, the host-only counts of a GFA
file (gbwt_hip_parse_gfa), the reader of the expected values against the fixtures, the metadata assembly (csrc/gfa_meta.hpp) as a program
of its own under ASan + UBSan, and the resources of the parse kernels."""
import ctypes as C
import os
import re
import subprocess

import pytest

import gbwt_rs_amd as G
import gfa_expect as X
import kat
import oracle_lib as O
from gbwt_rs_amd import _lib
from test_merge_cpu import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE, TRANSLATION = os.path.join(O.GOLDEN, "example.gfa"), os.path.join(O.GOLDEN, "translation.gfa")


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-C", _lib.CSRC], stdout=subprocess.DEVNULL)


def message():
    return _lib.lib().gbwt_hip_last_error().decode()


def test_bad_calls_are_refused_before_the_device():
    L = _lib.lib()
    h = C.c_void_p(1)
    assert L.gbwt_hip_build_from_gfa(None, 0, _lib.OPEN_ALL, C.byref(h)) == _lib.BAD_ARGUMENT and "null path" in message() and not h.value
    assert L.gbwt_hip_build_from_gfa(EXAMPLE.encode(), 0, _lib.OPEN_ALL, None) == _lib.BAD_ARGUMENT and "null output" in message()
    for flags in (0, 8, 15):
        h = C.c_void_p(1)
        assert L.gbwt_hip_build_from_gfa(EXAMPLE.encode(), 0, flags, C.byref(h)) == _lib.BAD_ARGUMENT and "flags" in message() and not h.value
        assert L.gbwt_hip_build_from_gfa_text(b"S\t1\tA\n", 6, 0, flags, C.byref(h)) == _lib.BAD_ARGUMENT and "flags" in message()
    h = C.c_void_p(1)
    assert L.gbwt_hip_build_from_gfa_text(None, 5, 0, _lib.OPEN_ALL, C.byref(h)) == _lib.BAD_ARGUMENT and "null text" in message() and not h.value
    assert L.gbwt_hip_build_from_gfa_text(b"x", 1, 0, _lib.OPEN_ALL, None) == _lib.BAD_ARGUMENT
    h = C.c_void_p(1)
    assert L.gbwt_hip_build_from_gfa(os.path.join(O.GOLDEN, "no-such-file.gfa").encode(), 0, _lib.OPEN_ALL, C.byref(h)) == _lib.IO_ERROR and "no-such-file" in message()
    assert not h.value
    assert L.gbwt_hip_last_gfa_info(None, None) == _lib.BAD_ARGUMENT
    assert L.gbwt_hip_parse_gfa(None, None) == _lib.BAD_ARGUMENT
    with pytest.raises(G.GbwtHipError) as e:
        G.parse_gfa(os.path.join(O.GOLDEN, "no-such-file.gfa"))
    assert e.value.status == _lib.IO_ERROR
    for method in ("from_gfa", "from_gfa_text", "last_gfa_info"):
        assert callable(getattr(G.GBZ, method)), method


COUNTS = ("bytes", "lines", "headers", "segments", "links", "p_lines", "w_lines", "ignored_lines", "steps", "label_bytes")


def test_parse_gfa_counts_the_fixtures():
    got = G.parse_gfa(EXAMPLE)
    assert [got[k] for k in COUNTS] == [os.path.getsize(EXAMPLE), 32, 1, 12, 13, 2, 4, 0, 28, 12]
    got = G.parse_gfa(TRANSLATION)
    assert [got[k] for k in COUNTS] == [os.path.getsize(TRANSLATION), 20, 1, 8, 8, 1, 2, 0, 15, 15]
    assert got["tile_bytes"] >= 16 and got["tile_bytes"] % 16 == 0 and got["peak_parse_bytes"] == 0


def test_parse_gfa_counts_ignored_and_empty_lines(tmp_path):
    text = (b"\n# a comment\nH\tVN:Z:1.1\tRS:Z:ref\n\n\nS\t1\tACGT\tLN:i:4\nS\t2\tC\nL\t1\t+\t2\t-\t0M\nE\tedge\nsomething else\n\t\n"
            b"P\tp\t1+,2-\nW\ts\t1\tc\t*\t5\t>1<2>1\nW\ts\t2\tc\t0\t0\t*\nP\tq\t*\t*\nx")          # no newline at the end
    path = tmp_path / "lines.gfa"
    path.write_bytes(text)
    got = G.parse_gfa(str(path))
    assert [got[k] for k in COUNTS] == [len(text), 13, 1, 2, 1, 2, 2, 5, 5, 5]
    want = X.Expected(text)
    assert (want.ignored, want.links, want.steps, len(want.paths), want.reference_samples) == (5, 1, 5, 4, "ref")
    path.write_bytes(b"S\t1\tA\nS\t2\tC\r\n")
    with pytest.raises(G.GbwtHipError) as e:
        G.parse_gfa(str(path))
    assert e.value.status == _lib.INVALID_DATA and "line 2" in str(e.value)


def test_expected_reader_on_the_fixtures():
    want = X.Expected(open(EXAMPLE, "rb").read())
    assert want.paths == kat.true_paths(False)[:2] + kat.true_paths(False)[2:]
    assert want.names == [(0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 1, 0), (1, 0, 2, 0), (1, 1, 1, 0), (1, 1, 2, 0)]
    assert (want.samples, want.contigs, want.haplotypes) == (["_gbwt_ref", "sample"], ["A", "B"], 3)
    with pytest.raises(X.Refused) as e:
        X.Expected(open(TRANSLATION, "rb").read())
    assert (e.value.line, e.value.status) == (2, X.UNSUPPORTED)


def test_metadata_assembly_under_sanitizers(tmp_path):
    """tests/cpp/gfa_meta.cpp: the name fields of example.gfa through assemble_gfa_metadata, built with ASan + UBSan and run as a program."""
    exe = tmp_path / "gfa_meta"
    subprocess.run([host_compiler(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", _lib.CSRC,
                    os.path.join(ROOT, "tests", "cpp", "gfa_meta.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), EXAMPLE], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert not any(line.startswith("FAIL") for line in lines), out.stdout
    assert lines[0] == "counts 2 3 2 7 6"                     # samples, haplotypes, contigs, flags, paths: the header of example.meta
    assert [tuple(int(x) for x in line.split()[1:]) for line in lines if line.startswith("path ")] == \
        [(0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 1, 0), (1, 0, 2, 0), (1, 1, 1, 0), (1, 1, 2, 0)]
    rest = {line.split(" ", 1)[0]: line.split(" ", 1)[1] for line in lines if " " in line and not line.startswith(("path ", "counts "))}
    assert rest["samples"] == "_gbwt_ref sample" and rest["contigs"] == "A B" and rest["generic_on_disk"] == "1"
    assert rest["rs"] == "a b" and rest["rs_absent"] == "0"
    assert rest["star"] == "0 7 refused 0"
    assert rest["duplicate"] == "5" and rest["duplicate_behind_stop"] == "0"
    assert rest["hap"] == "7"                                 # the earlier of two bad lines
    assert rest["counts_host"] == "32 12 13 2 4 28 12"


def test_parse_kernels_compile_without_scratch():
    """Every kernel of gfa_parse.hip for gfx950: nothing spilled, no scratch."""
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                          os.path.join(_lib.CSRC, "gfa_parse.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = set()
    for at, line in enumerate(lines):
        if "Function Name" in line and "k_gfa_" in line:
            block = "\n".join(lines[at:at + 14])
            assert int(re.search(r"VGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"SGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)) == 0, block
            seen.add(re.search(r"(k_gfa_[a-z_]+?)E", line).group(1))
    for kernel in ("k_gfa_count_structure", "k_gfa_record_structure", "k_gfa_lines", "k_gfa_gather_lines", "k_gfa_count_steps", "k_gfa_fill_steps", "k_gfa_duplicates",
                   "k_gfa_label_slots", "k_gfa_copy_labels"):
        assert kernel in seen, (kernel, sorted(seen))
