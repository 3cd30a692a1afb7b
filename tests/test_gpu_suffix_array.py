"""Suffix array and BWT of a text on the device (csrc/suffix_array.hip), against yardsticks built without the library: the brute-force sort
of tests/tags_expect.py on short texts, the independent prefix doubling and the linear certificate of tests/sa_expect.py on longer ones.
The chain `sequences` -> suffix array -> `tag-array` of gbz-extract runs through files the library wrote itself."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import gbwt_rs_amd as G
import oracle_lib as O
import sa_expect as A
import seq_expect as E
import tags_expect as T
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S
from test_gpu_tags import FIXTURES, fixture_text

pytestmark = pytest.mark.gpu

SMALL = A.small_texts()
GUARD = 0x5A


@functools.lru_cache(maxsize=None)
def brute(text):
    sa = T.suffix_array(text)
    sa.setflags(write=False)
    return sa


def device_form(text, sentinel, lead):
    """gbwt_hip_suffix_array_text_device over torch buffers with `lead` guard bytes in front of the text and of the BWT (1: neither is
    aligned) and guard words around the suffix array: (sa, bwt, runs), after checking that the guards are untouched."""
    import torch
    n = len(text)
    dev = torch.device("cuda", 0)
    d_text = torch.from_numpy(np.frombuffer(b"\x5a" * lead + text + b"\x5a" * 8, dtype=np.uint8).copy()).to(dev)
    d_sa = torch.full((n + 2,), -1, dtype=torch.int64, device=dev)
    d_bwt = torch.full((n + lead + 8,), GUARD, dtype=torch.uint8, device=dev)
    runs = C.c_uint64(0)
    _lib.check(_lib.lib().gbwt_hip_suffix_array_text_device(0, C.c_void_p(d_text.data_ptr() + lead), n, sentinel, C.c_void_p(d_sa.data_ptr() + 8), C.c_void_p(d_bwt.data_ptr() + lead),
                                                            None, C.byref(runs)))
    sa, bwt = d_sa.cpu().numpy().view(np.uint64), d_bwt.cpu().numpy()
    assert sa[0] == sa[-1] == 0xFFFFFFFFFFFFFFFF and (bwt[:lead] == GUARD).all() and (bwt[lead + n:] == GUARD).all()
    return sa[1:-1], bwt[lead:lead + n], runs.value


@pytest.mark.parametrize("name,text", SMALL, ids=[name for name, _ in SMALL])
def test_text_level_against_the_brute_force_sort(name, text):
    want = brute(text)
    n = len(text)
    for sentinel in (0, 36, 255):
        want_bwt = A.bwt(text, want, sentinel)
        sa, bwt, runs = G.suffix_array_text(text, sentinel=sentinel, return_bwt=True)
        assert sa.dtype == np.uint64 and np.array_equal(sa, want), (name, sentinel)
        assert np.array_equal(bwt, want_bwt) and runs == A.runs(want_bwt), (name, sentinel)
        info = G.last_suffix_array_info()
        assert info["n"] == n and info["bwt_runs"] == runs and info["peak_scratch_bytes"] == info["planned_scratch_bytes"]
        for lead in (1, 16):                                                  # the device-pointer form: the same bytes, nothing outside them
            d_sa, d_bwt, d_runs = device_form(text, sentinel, lead)
            assert np.array_equal(d_sa, want) and np.array_equal(d_bwt, want_bwt) and d_runs == runs, (name, sentinel, lead)
    assert np.array_equal(G.suffix_array_text(text), want)                    # without the BWT
    if n:
        active = info["active"]
        assert len(active) == info["rounds"] + 1 and active[-1] == 0 and all(a >= b for a, b in zip(active, active[1:]))
        assert info["rounds"] <= math.ceil(math.log2(n)) + 1
    if name == "a_run":                                                       # every round leaves all but the suffixes it has reached tied
        assert info["rounds"] >= 8 and active[0] >= n - 16 and active[info["rounds"] - 1] > 0


def test_repetitive_text_against_doubling_and_check():
    text = A.mutated_rows(60, 5000, 5)
    assert len(text) == 300060
    want = A.doubling(text)
    assert A.check(text, want) is None
    sa, bwt, runs = G.suffix_array_text(text, return_bwt=True)
    assert A.check(text, sa) is None and np.array_equal(sa, want)
    assert np.array_equal(bwt, A.bwt(text, want)) and runs == A.runs(bwt)
    info = G.last_suffix_array_info()
    active = info["active"]
    assert all(a >= b for a, b in zip(active, active[1:])) and info["rounds"] > 2 and active[2] > 0 and active[-1] == 0
    assert info["rounds"] <= math.ceil(math.log2(len(text))) + 1
    # random bases: of the n^2 / 2 = 4.5e10 pairs of suffixes one in 4^14 = 2.7e8 agrees on 14 bytes -- some 170 pairs stay tied behind round 1 --
    # and one in 4^28 = 7.2e16 on 28: round 2 leaves nothing
    rng = np.random.default_rng(17)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=300000)].tobytes()
    sa = G.suffix_array_text(text)
    assert A.check(text, sa) is None
    info = G.last_suffix_array_info()
    assert info["rounds"] == 2 and info["active"][0] > info["active"][1] > 0 and info["active"][2] == 0


def test_three_million_positions_by_the_certificate():
    text = A.mutated_rows(60, 50000, 5)
    n = len(text)
    assert n == 3000060
    sa, bwt, runs = G.suffix_array_text(text, sentinel=36, return_bwt=True)
    assert A.check(text, sa) is None
    assert np.array_equal(bwt, A.bwt(text, sa, 36)) and runs == A.runs(bwt)
    info = G.last_suffix_array_info()
    print(f"peak_scratch_bytes / n = {info['peak_scratch_bytes'] / n:.2f}, planned {info['planned_scratch_bytes'] / n:.2f}, rounds {info['rounds']}, active {info['active']}")
    assert 0 < info["peak_scratch_bytes"] == info["planned_scratch_bytes"]    # what sa_plan promised: everything is allocated up front
    assert info["rounds"] <= math.ceil(math.log2(n)) + 1 and info["rank_bits"] == 22


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_fixtures(name):
    import torch
    path = os.path.join(O.GOLDEN, name)
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    translated = bool(G.parse_file(path).has_translation)
    lengths, _ = fixture_text(dev, oracle, translated)
    ids = list(range(dev.paths()))
    for order in (ids, ids[::-1], ids[::-1] + ids[:1]):
        tag_text, offsets = T.oracle_text(oracle, order, lengths)
        for endmarker in (0, 36, 255, None):
            _, data = dev.path_sequences(order, endmarker=endmarker)
            want = brute(bytes(data))
            sentinel = 0 if endmarker is None else endmarker
            sa, bwt, runs = dev.suffix_array(order, endmarker=endmarker, return_bwt=True)
            assert np.array_equal(sa, want), (order, endmarker)
            assert np.array_equal(bwt, A.bwt(data, want, sentinel)) and runs == A.runs(bwt), (order, endmarker)
            assert np.array_equal(dev.suffix_array(order, endmarker=endmarker), want)
            out = dev.suffix_array_device(order, endmarker=endmarker)
            assert out.total == len(data) and out.bwt_runs == runs
            if endmarker is None:
                continue
            # the device result is a suffix array for the tag kernel as it lies there
            assert out.total == tag_text.size == int(offsets[-1])
            d_tags = torch.full((out.total + 2,), -1, dtype=torch.int64, device="cuda:0")
            tag_runs = dev.tags_device(order, out.d_sa, out.total, d_tags.data_ptr() + 8)
            tags = d_tags.cpu().numpy().view(np.uint64)
            want_tags = T.gather(tag_text, want)
            assert np.array_equal(tags[1:-1], want_tags) and tag_runs == T.runs(want_tags), (order, endmarker)
            assert tags[0] == tags[-1] == 0xFFFFFFFFFFFFFFFF
    assert dev.suffix_array([]).size == 0 and dev.suffix_array_device([]).total == 0


def test_files_chain_sequences_suffix_array_tags(tmp_path):
    gbz = str(tmp_path / "genome.gbz")
    S.Synth.genome(contigs=2, fragments=2, haplotypes=16, sites=40, labels=1).save(gbz, as_gbz=True)
    dev, oracle = G.GBZ.load(gbz), O.OracleGBZ(gbz)
    ids = np.arange(dev.paths(), dtype=np.uint64)
    base = str(tmp_path / "out")
    dev.write_sequences(base)
    text = open(base, "rb").read()
    assert len(text) == dev.text_length(ids) and text[-1] == 0
    want = A.doubling(text)
    assert A.check(text, want) is None
    runs = dev.write_suffix_array(base)
    want_bwt = A.bwt(text, want, 0)
    assert open(base + ".sa", "rb").read() == np.concatenate([[len(text)], want]).astype("<u8").tobytes()
    bwt_file = open(base + ".bwt", "rb").read()
    assert bwt_file == text[-1:] + want_bwt.tobytes()
    assert runs == A.runs(np.frombuffer(bwt_file, dtype=np.uint8)[1:]) == A.runs(want_bwt)
    # tag-array mode at its defaults reads them as they are
    tag_text, _ = T.oracle_text(oracle, ids, E.LabelTable.from_gfa(oracle.gfa()).len)
    want_tags = T.gather(tag_text, want)
    assert dev.write_tag_array(base) == T.runs(want_tags)
    assert open(base + ".tags", "rb").read() == want_tags.astype("<u8").tobytes()
    # another endmarker is read from the end of `base`
    dev.write_sequences(base, endmarker=36)
    text = open(base, "rb").read()
    assert text[-1] == 36
    want = A.doubling(text)
    assert dev.write_suffix_array(base) == A.runs(A.bwt(text, want, 36))
    assert open(base + ".sa", "rb").read() == np.concatenate([[len(text)], want]).astype("<u8").tobytes()
    assert open(base + ".bwt", "rb").read() == b"$" + A.bwt(text, want, 36).tobytes()
    # failures leave neither file behind: not half written ones, and not those of an earlier call, which would no longer match the names
    names = open(base + ".names").read()

    def failing(status, message):
        for suffix in (".sa", ".bwt"):
            if not os.path.exists(base + suffix):
                open(base + suffix, "wb").write(b"left by an earlier call")
        with pytest.raises(G.GbwtHipError) as e:
            dev.write_suffix_array(base)
        assert e.value.status == status and message in str(e.value), str(e.value)
        assert not os.path.exists(base + ".sa") and not os.path.exists(base + ".bwt")

    lines = names.splitlines()
    f = lines[2].split("\t")
    open(base + ".names", "w").write("\n".join(lines[:2] + ["\t".join(f[:5] + [str(int(f[5]) + 1)])] + lines[3:]) + "\n")
    os.rename(base, base + ".text")                                           # (so that the lengths are checked against the walk, not the file)
    failing(_lib.INVALID_DATA, f"Invalid length for path {f[0]}: expected {int(f[5]) + 1}, got {int(f[5])}")
    os.rename(base + ".text", base)
    failing(_lib.INVALID_DATA, "bytes")                                       # the size of `base` against the names
    open(base + ".names", "w").write(names)
    open(base, "ab").write(b"A")
    failing(_lib.INVALID_DATA, "bytes")
    os.remove(base + ".names")
    failing(_lib.IO_ERROR, "cannot open")


def test_one_reader_of_the_names_for_both_modes(tmp_path):
    """`base`.names is read by one piece of code (csrc/extract_files.hpp): the suffix array mode and the tag-array mode refuse a malformed
    or mismatching file with the same status and the same words -- before either looks for `base`.sa -- and agree on a reordered one."""
    path = os.path.join(O.GOLDEN, "example.gbz")
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    n = dev.paths()
    base = str(tmp_path / "example")
    dev.write_sequences(base)
    names = open(base + ".names").read()
    os.remove(base)                                                           # (so that the lengths are checked against the walk, not the file)
    lines = names.splitlines()
    f = lines[2].split("\t")
    wrong = "\n".join(lines[:2] + ["\t".join(f[:5] + [str(int(f[5]) + 1)])] + lines[3:]) + "\n"
    cases = [("", "No path names found"),
             (names.replace("\t", " "), "Name line missing last field"),
             (f"{n}\tx\ty\t0\t0\t5\n", f"Invalid length for path {n}: expected 5, got 0 (no such path)"),
             (wrong, f"Invalid length for path 2: expected {int(f[5]) + 1}, got {int(f[5])}")]
    for text, message in cases:
        open(base + ".names", "w").write(text)
        seen = []
        for call in (dev.write_tag_array, dev.write_suffix_array):
            with pytest.raises(G.GbwtHipError) as e:
                call(base)
            seen.append((e.value.status, dev._L.gbwt_hip_last_error().decode()))
        assert seen[0] == seen[1] and seen[0] == (_lib.INVALID_DATA, message), seen
        assert not any(os.path.exists(base + suffix) for suffix in (".sa", ".bwt", ".tags"))
    # two fields, another order, no final newline: the suffix array one mode writes is the one the other reads to its end
    open(base + ".names", "w").write("5\t4\n0\tanything\t5")
    _, data = dev.path_sequences([5, 0], endmarker=0)
    want = brute(bytes(data))
    dev.write_suffix_array(base)
    assert open(base + ".sa", "rb").read() == np.concatenate([[len(data)], want]).astype("<u8").tobytes()
    part, _ = T.oracle_text(oracle, [5, 0])
    want_tags = T.gather(part, want)
    assert dev.write_tag_array(base) == T.runs(want_tags)
    assert open(base + ".tags", "rb").read() == want_tags.astype("<u8").tobytes()


def test_workspace_memo_memory_and_guards():
    path = os.path.join(O.GOLDEN, "example.gbz")
    dev = G.GBZ.load(path)
    ids = np.arange(dev.paths(), dtype=np.uint64)
    with pytest.raises(G.GbwtHipError) as e:
        dev.last_suffix_array_info()
    assert e.value.status == _lib.BAD_ARGUMENT
    before = dev.memory_usage()["workspace_device_bytes"]
    total, runs = C.c_uint64(0), C.c_uint64(0)
    _lib.check(dev._L.gbwt_hip_path_suffix_array(dev._h, dev._ws, ids.ctypes.data, ids.size, 0, None, None, 0, C.byref(total), C.byref(runs)))   # the size query builds
    assert total.value == dev.text_length(ids) == 34
    first = dev.last_suffix_array_info()
    assert first["n"] == 34 and first["pack_ms"] > 0 and first["rank_ms"] > 0 and first["output_ms"] > 0 and first["text_ms"] > 0
    assert dev.memory_usage()["workspace_device_bytes"] - before >= 9 * total.value
    sa = np.zeros(34, dtype=np.uint64)
    short = C.c_uint64(0)
    assert dev._L.gbwt_hip_path_suffix_array(dev._h, dev._ws, ids.ctypes.data, ids.size, 0, sa.ctypes.data, None, 33, C.byref(short), None) == _lib.CAPACITY and short.value == 34
    _lib.check(dev._L.gbwt_hip_path_suffix_array(dev._h, dev._ws, ids.ctypes.data, ids.size, 0, sa.ctypes.data, None, 34, C.byref(total), C.byref(runs)))   # the fill only copies
    assert dev.last_suffix_array_info() == first
    _, data = dev.path_sequences(ids, endmarker=0)
    assert np.array_equal(sa, brute(bytes(data)))
    assert dev.suffix_array_device(ids).total == 34 and dev.last_suffix_array_info() == first     # the device form finds it as well
    # requests of other families in between do not disturb it; another request replaces it
    dev.sequences_csr([0, 1])
    dev.path_sequences([1], endmarker=0)
    assert np.array_equal(dev.suffix_array(ids), sa) and dev.last_suffix_array_info() == first
    assert dev.suffix_array(ids, endmarker=36).size == 34 and dev.last_suffix_array_info() != first
    # guards: as the bases calls
    out = _lib.SuffixArray()
    assert dev._L.gbwt_hip_path_suffix_array_device(dev._h, dev._ws, ids.ctypes.data, ids.size, 256, C.byref(out)) == _lib.BAD_ARGUMENT
    assert dev._L.gbwt_hip_path_suffix_array_device(dev._h, dev._ws, ids.ctypes.data, ids.size, -2, C.byref(out)) == _lib.BAD_ARGUMENT
    assert dev._L.gbwt_hip_path_suffix_array_device(dev._h, dev._ws, None, 2, 0, C.byref(out)) == _lib.BAD_ARGUMENT
    gbwt = G.GBWT.load(os.path.join(O.GOLDEN, "example.gbwt"))
    one = np.zeros(1, dtype=np.uint64)
    assert gbwt._L.gbwt_hip_path_suffix_array_device(gbwt._h, gbwt._ws, one.ctypes.data, 1, 0, C.byref(out)) == _lib.BAD_ARGUMENT
    assert gbwt._L.gbwt_hip_write_suffix_array(gbwt._h, gbwt._ws, b"/nonexistent/base", None) == _lib.BAD_ARGUMENT
    search_only = G.GBZ.load(path, flags=_lib.OPEN_SEARCH)
    with pytest.raises(G.GbwtHipError) as e:
        search_only.suffix_array([0])
    assert e.value.status == _lib.BAD_ARGUMENT
    other = dev.another_workspace()
    assert dev._L.gbwt_hip_path_suffix_array_device(dev._h, None, one.ctypes.data, 1, 0, C.byref(out)) == _lib.BAD_ARGUMENT
    assert other.suffix_array([0]).size == dev.text_length([0])
