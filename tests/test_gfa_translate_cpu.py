"""Construction from GFA with a node-to-segment translation, without a GPU: the reader of the expected values (gfa_translate_expect.py)
against translation.gbz -- a file the upstream tool made from translation.gfa with --max-node 2 --, the name table (csrc/gfa_names.hpp)
as a program of its own under ASan + UBSan, and the argument checks that answer before the device is touched."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import gfa_expect as X
import gfa_translate_expect as T
import oracle_lib as O
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S
from test_merge_cpu import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE, TRANSLATION = os.path.join(O.GOLDEN, "example.gfa"), os.path.join(O.GOLDEN, "translation.gfa")


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-C", _lib.CSRC], stdout=subprocess.DEVNULL)


def test_reader_on_the_translation_fixture():
    want = T.Translated(open(TRANSLATION, "rb").read(), max_node=2)
    assert want.translated
    first, second = [1, 2, 3, 5, 6, 9, 11], [1, 2, 4, 5, 6, 10, 11]
    assert want.paths == [[2 * v for v in row] for row in (first, first, second)]
    known = json.load(open(os.path.join(O.GOLDEN, "graph_known.json")))["translation.gbz"]
    assert want.segments == known["segments"]
    assert (want.samples, want.contigs, want.names) == (["_gbwt_ref", "sample"], ["A"], [(0, 0, 0, 0), (1, 0, 1, 0), (1, 0, 2, 0)])


def test_rows_of_the_reader_are_the_records_of_the_fixture():
    """Synth.from_paths over the reader's rows = the GBWT gfa2gbwt wrote."""
    want = T.Translated(open(TRANSLATION, "rb").read(), max_node=2)
    mine = S.Synth.from_paths(want.paths, bidirectional=True)
    ref = O.OracleGBZ(os.path.join(O.GOLDEN, "translation.gbz")).gbwt()
    assert (mine.sequences, mine.size, mine.alphabet_offset, mine.alphabet_size) == (ref.sequences(), ref.len(), ref.alphabet_offset(), ref.alphabet_size())
    bwt = ref.bwt()
    assert bytes(mine.data()) == bwt.data() and list(mine.starts()) == bwt.starts()


def test_reader_modes():
    text = open(EXAMPLE, "rb").read()
    plain = T.Translated(text, max_node=1024, translate=T.AUTO)                # nothing to translate: the untranslated reader's answer
    assert not plain.translated and plain.paths == X.Expected(text).paths
    always = T.Translated(text, max_node=0, translate=T.ALWAYS)
    assert always.translated and [row[1] for row in always.segments] == [str(v) for v in (11, 12, 13, 14, 15, 16, 17, 21, 22, 23, 24, 25)]
    assert [row[2:4] for row in always.segments] == [[k, k + 1] for k in range(1, 13)]
    chopped = T.Translated("S\ta\tACGTA\nS\tb\tAC\nS\tc\tA\nP\tp\ta-,c+\n", max_node=2)
    assert chopped.segments == [[0, "a", 1, 4, "ACGTA"], [1, "", 4, 5, ""], [2, "c", 5, 6, "A"]]
    assert chopped.paths == [[7, 5, 3, 10]] and chopped.node_labels == {1: b"AC", 2: b"GT", 3: b"A", 4: b"", 5: b"A"}
    for bad, line, status in (("S\ta\tA\nS\tb\tC\nS\ta\tG\n", 3, X.INVALID_DATA), ("S\t" + "n" * 256 + "\tA\n", 1, X.UNSUPPORTED), ("S\ta\tA\nP\tp\ta+,,a+\n", 2, X.INVALID_DATA),
                              ("S\ta\tA\nW\ts\t1\tc\t0\t1\t>a>>a\n", 2, X.INVALID_DATA), ("S\ta\tA\nP\tp\ta+,b+\n", 2, X.INVALID_DATA), ("S\ta\tA\nP\tp\ta\n", 2, X.INVALID_DATA),
                              ("S\ta\tA\nW\ts\t1\tc\t0\t1\ta>a\n", 2, X.INVALID_DATA), ("S\ta\tA\nP\tp\ta+,\n", 2, X.INVALID_DATA)):
        with pytest.raises(X.Refused) as e:
            T.Translated(bad, max_node=2)
        assert (e.value.line, e.value.status) == (line, status), bad


def test_name_table_under_sanitizers(tmp_path):
    """tests/cpp/gfa_names.cpp: hash, buckets, lookup and the duplicate check of csrc/gfa_names.hpp with the real hash and with a constant
    one, built with ASan + UBSan and run as a program."""
    exe = tmp_path / "gfa_names"
    subprocess.run([host_compiler(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", _lib.CSRC,
                    os.path.join(ROOT, "tests", "cpp", "gfa_names.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert not any(line.startswith("FAIL") for line in lines), out.stdout
    assert lines[-1] == "failures 0"
    assert [line for line in lines if line.startswith("constant ")] == ["constant buckets 16 longest 12 bits 4"]      # every name in one bucket


def message():
    return _lib.lib().gbwt_hip_last_error().decode()


def test_bad_options_are_refused_before_the_device():
    L = _lib.lib()
    text = b"S\t1\tA\n"
    cases = {"max_node_length": _lib.GfaOptions(2, _lib.GFA_TRANSLATE_NEVER), "translate": _lib.GfaOptions(0, 3), "reserved": _lib.GfaOptions(0, _lib.GFA_TRANSLATE_AUTO, (0, 1)),
             "reserved ": _lib.GfaOptions(2, _lib.GFA_TRANSLATE_ALWAYS, (1, 0))}
    for word, opts in cases.items():
        h = C.c_void_p(1)
        assert L.gbwt_hip_build_from_gfa_text_opts(text, len(text), C.byref(opts), 0, _lib.OPEN_ALL, C.byref(h)) == _lib.BAD_ARGUMENT and word.strip() in message() and not h.value
        h = C.c_void_p(1)
        assert L.gbwt_hip_build_from_gfa_opts(TRANSLATION.encode(), C.byref(opts), 0, _lib.OPEN_ALL, C.byref(h)) == _lib.BAD_ARGUMENT and word.strip() in message() and not h.value
    good = _lib.GfaOptions(2, _lib.GFA_TRANSLATE_AUTO)
    h = C.c_void_p(1)
    assert L.gbwt_hip_build_from_gfa_opts(None, C.byref(good), 0, _lib.OPEN_ALL, C.byref(h)) == _lib.BAD_ARGUMENT and "null path" in message() and not h.value
    assert L.gbwt_hip_build_from_gfa_text_opts(text, len(text), C.byref(good), 0, 0, C.byref(h)) == _lib.BAD_ARGUMENT and "flags" in message()
    assert L.gbwt_hip_build_from_gfa_text_opts(text, len(text), C.byref(good), 0, _lib.OPEN_ALL, None) == _lib.BAD_ARGUMENT
    h = C.c_void_p(1)
    assert L.gbwt_hip_build_from_gfa_opts(os.path.join(O.GOLDEN, "no-such-file.gfa").encode(), C.byref(good), 0, _lib.OPEN_ALL, C.byref(h)) == _lib.IO_ERROR and not h.value
    assert L.gbwt_hip_last_gfa_translation_info(None, None) == _lib.BAD_ARGUMENT


def test_translation_kernels_compile_without_scratch():
    """The kernels a translated parse adds to gfa_parse.hip, for gfx950: nothing spilled, no scratch, no LDS."""
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
            assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", block).group(1)) == 0, block
            seen.add(re.search(r"(k_gfa_[a-z_]+?)E", line).group(1))
    for kernel in ("k_gfa_segment_plan", "k_gfa_name_duplicates", "k_gfa_name_buckets", "k_gfa_count_tokens", "k_gfa_fill_tokens", "k_gfa_path_offsets", "k_gfa_expand_steps",
                   "k_gfa_node_slots", "k_gfa_name_slots"):
        assert kernel in seen, (kernel, sorted(seen))
