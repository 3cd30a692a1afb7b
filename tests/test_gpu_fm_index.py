"""The FM-index over a text on the device (csrc/fm_index.hip, csrc/capi_fm.hip) against tests/fm_expect.py -- occurrences by startswith at
every position, looked up in the brute-force suffix array -- at text level, and against the library's own tag_array of the true suffix
array at path level."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fm_expect as F
import gbwt_rs_amd as G
import oracle_lib as O
import sa_expect as A
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S
from test_gpu_tags import FIXTURES

pytestmark = pytest.mark.gpu

SMALL = A.small_texts()
GUARD = 0x5A


@functools.lru_cache(maxsize=None)
def brute(text):
    sa = F.suffix_array(text)
    sa.setflags(write=False)
    return sa


@functools.lru_cache(maxsize=None)
def expected(text, patterns):
    """(ranges, rows) of a tuple of patterns: computed once per text, shared by the sentinels and the tests."""
    return F.expected(text, brute(text), list(patterns))


def rows_of(offsets, values):
    return [values[int(offsets[k]):int(offsets[k + 1])] for k in range(offsets.size - 1)]


def check_index(fm, text, patterns, what):
    want_ranges, want_rows = expected(text, tuple(patterns))
    ranges = fm.count(patterns)
    assert ranges.dtype == np.uint64 and ranges.shape == (len(patterns), 2)
    assert np.array_equal(ranges.astype(np.int64), want_ranges), (what, [(p, r, w) for p, r, w in zip(patterns, ranges.tolist(), want_ranges.tolist()) if r != w][:5])
    offsets, positions = fm.locate_csr(patterns)
    assert offsets[0] == 0 and np.array_equal(np.diff(offsets.astype(np.int64)), want_ranges[:, 1] - want_ranges[:, 0]), what
    for p, got, want in zip(patterns, rows_of(offsets, positions), want_rows):
        assert np.array_equal(got, want), (what, p)


@pytest.mark.parametrize("name,text", SMALL, ids=[name for name, _ in SMALL])
def test_small_texts_against_brute_force(name, text):
    patterns = F.text_patterns(text)
    n = len(text)
    assert len(patterns) % 64 != 0 and (n < 9 or [len(p) for p in patterns[1:5]] == [1, 2, 3, 9])     # neighbours in a wave differ in length
    for sentinel in (0, 65, 255):
        fm = G.FMIndex.from_text(text, sentinel=sentinel)
        info = fm.info()
        assert info["n"] == n and info["sigma"] == len(set(text)) and info["packed"] == (info["sigma"] <= 8) and info["block_rows"] == (96 if info["packed"] else 256)
        assert info["blocks"] == (n + 1) // info["block_rows"] + 1 and info["index_bytes"] == info["planned_index_bytes"]
        if n:
            assert info["primary"] == int(np.flatnonzero(brute(text) == 0)[0])
        check_index(fm, text, patterns, (name, sentinel))
        ranges = fm.count([b"", text + b"A", b"\0\0\0\0ZZ"])
        assert ranges[0].tolist() == [0, n] and ranges[1].tolist() == [0, 0] and ranges[2].tolist() == [0, 0]
        if name == "a_run":
            ks = (1, 64, 4999, 5000)
            ranges = fm.count([b"A" * k for k in ks])
            assert (ranges[:, 1] - ranges[:, 0]).tolist() == [5000 - k + 1 for k in ks]
            assert fm.locate(b"A" * 4999).tolist() == [1, 0] and fm.count([b"A" * 5001]).tolist() == [[0, 0]]
        assert fm.count([]).shape == (0, 2) and fm.locate_csr([])[0].tolist() == [0]
        fm.close()


def kmers(text, k, count, rng):
    at = rng.integers(0, len(text) - k + 1, size=count)
    return [text[i:i + k] for i in at]


@pytest.mark.parametrize("letters", [b"ACGT", b"ACGTNRYKMSWB"], ids=["packed", "plain"])
def test_block_edges(letters):
    rng = np.random.default_rng(23)
    alphabet = np.frombuffer(letters, dtype=np.uint8)
    probe = G.FMIndex.from_text(bytes(alphabet))
    B = probe.info()["block_rows"]
    assert B == (96 if len(letters) <= 8 else 256) and probe.info()["packed"] == (len(letters) <= 8)
    probe.close()
    short = [bytes([a]) for a in alphabet[:4]] + [bytes([a, b]) for a in alphabet[:4] for b in alphabet[:4]] + [bytes(alphabet[-2:]), bytes(alphabet[-1:])]
    for n in (B - 1, B, B + 1, 2 * B, 2 * B + 1):
        text = alphabet[rng.integers(0, alphabet.size, size=n)].tobytes()
        fm = G.FMIndex.from_text(text, sentinel=65)
        assert fm.info()["blocks"] == (n + 1) // B + 1
        check_index(fm, text, short + kmers(text, 9, 64, rng), (letters, n))
        fm.close()


def test_all_byte_values():
    text = dict(SMALL)["all_bytes"]
    rng = np.random.default_rng(29)
    fm = G.FMIndex.from_text(text, sentinel=255)
    info = fm.info()
    assert info["sigma"] == 256 and not info["packed"] and info["block_rows"] == 256
    patterns = [bytes([b]) for b in range(256)] + kmers(text, 2, 150, rng) + kmers(text, 3, 150, rng) + [b"\xff\xff\xff\xff"]
    check_index(fm, text, patterns, "all_bytes")
    ranges = fm.count([bytes([b]) for b in range(256)])
    assert (ranges[:, 1] - ranges[:, 0]).tolist() == np.bincount(np.frombuffer(text, dtype=np.uint8), minlength=256).tolist()
    fm.close()


def test_count_only():
    text = A.mutated_rows(6, 500, 3)
    patterns = F.text_patterns(text[:700]) + kmers(text, 12, 50, np.random.default_rng(31))
    full, lean = G.FMIndex.from_text(text), G.FMIndex.from_text(text, count_only=True)
    assert np.array_equal(full.count(patterns), lean.count(patterns))
    assert np.array_equal(full.count(patterns).astype(np.int64), expected(text, tuple(patterns))[0])
    with pytest.raises(G.GbwtHipError) as e:
        lean.locate_csr(patterns)
    assert e.value.status == _lib.UNSUPPORTED
    a, b = full.info(), lean.info()
    assert b["count_only"] == 1 and b["sa_bytes"] == 0 and a["sa_bytes"] == 4 * len(text) and a["index_bytes"] - b["index_bytes"] == 4 * len(text)
    assert b["index_bytes"] == b["planned_index_bytes"] == (len(text) + 1) // 96 * 128 + 128 + 1536
    full.close()
    lean.close()


def guarded(array, dtype, lead):
    """`array` in device memory with `lead` guard bytes in front and 16 behind: (tensor, device pointer of the payload)."""
    import torch
    raw = np.concatenate([np.full(lead, GUARD, np.uint8), np.ascontiguousarray(array).view(np.uint8).reshape(-1), np.full(16, GUARD, np.uint8)])
    t = torch.from_numpy(raw).to("cuda:0")
    return t, t.data_ptr() + lead


def view(pointer, count, device="cuda:0"):
    import torch
    from gbwt_rs_amd import dist as D
    return D.device_view(pointer, count * 8, torch.uint8, torch.device(device)).cpu().numpy().view(np.uint64).copy()


def test_device_forms():
    import torch
    text = A.mutated_rows(4, 300, 3) + b"ACGTTGCA"
    patterns = F.text_patterns(text)
    offsets, data = G.api._patterns_csr(patterns)
    m = len(patterns)
    want_sa = brute(text)
    host = G.FMIndex.from_text(text)
    h_ranges = host.count(patterns)
    h_offsets, h_positions = host.locate_csr(patterns)
    # the text and a suffix array made by the caller, in torch buffers; and the same with a NULL suffix array
    t_text, p_text = guarded(np.frombuffer(text, dtype=np.uint8), np.uint8, 1)
    t_sa, p_sa = guarded(want_sa, np.uint64, 8)
    t_off, p_off = guarded(offsets, np.uint64, 8)
    t_dat, p_dat = guarded(data, np.uint8, 3)
    torch.cuda.synchronize()
    for d_sa in (p_sa, None):
        fm = G.FMIndex.from_device(p_text, len(text), sentinel=65, d_sa=d_sa)
        counted = fm.count_device(p_off, p_dat, m, data.size)
        assert counted.m == m and np.array_equal(view(counted.d_ranges, 2 * m).reshape(m, 2), h_ranges)
        located = fm.locate_device(p_off, p_dat, m, data.size)
        assert located.m == m and located.total == h_positions.size
        assert np.array_equal(view(located.d_offsets, m + 1), h_offsets) and np.array_equal(view(located.d_values, located.total), h_positions)
        assert np.array_equal(view(located.d_ranges, 2 * m).reshape(m, 2), h_ranges)
        assert np.array_equal(fm.count(patterns), h_ranges)                    # the host form on the same object
        # offsets that leave the pattern bytes are found by the kernel
        with pytest.raises(G.GbwtHipError) as e:
            fm.count_device(p_off, p_dat, m, data.size - 1)
        assert e.value.status == _lib.BAD_ARGUMENT
        fm.close()
    for t, lead, payload in ((t_text, 1, len(text)), (t_sa, 8, 8 * len(text)), (t_off, 8, 8 * (m + 1)), (t_dat, 3, data.size)):
        raw = t.cpu().numpy()
        assert (raw[:lead] == GUARD).all() and (raw[lead + payload:] == GUARD).all() and raw.size == lead + payload + 16
    assert np.array_equal(t_sa.cpu().numpy()[8:-16].view(np.uint64), want_sa)
    # a suffix array that is none: a value outside the text
    bad = want_sa.copy()
    bad[3] = len(text)
    t_bad, p_bad = guarded(bad, np.uint64, 8)
    torch.cuda.synchronize()
    with pytest.raises(G.GbwtHipError) as e:
        G.FMIndex.from_device(p_text, len(text), d_sa=p_bad)
    assert e.value.status == _lib.INVALID_DATA
    host.close()


def path_patterns(text, dev):
    text = bytes(text)
    found = set()
    for k in (1, 3, 5):
        found.update(text[i:i + k] for i in range(len(text) - k + 1))
    for v in range(1, dev.alphabet_size() // 2 + 1):
        label = dev.node_sequence(v)
        if label is not None and 0 < len(label) <= 16:
            found.add(bytes(label))
    return sorted(found)


def check_paths(dev, what):
    ids = np.arange(dev.paths(), dtype=np.uint64)
    _, text = dev.path_sequences(ids, endmarker=0)
    text = bytes(text)
    sa = brute(text)
    tags = dev.tag_array(ids, sa)
    patterns = path_patterns(text, dev)
    fm = dev.fm_index(ids)
    info = fm.info()
    assert info["path_level"] == 1 and info["n"] == len(text) and info["suffix_array_ms"] == 0
    want_ranges, _ = expected(text, tuple(patterns))
    assert np.array_equal(fm.count(patterns).astype(np.int64), want_ranges), what
    offsets, got = fm.graph_positions_csr(patterns, unique=False)
    u_offsets, u_got = fm.graph_positions_csr(patterns, unique=True)
    assert np.array_equal(np.diff(offsets.astype(np.int64)), want_ranges[:, 1] - want_ranges[:, 0])
    for k, (p, (lo, hi)) in enumerate(zip(patterns, want_ranges)):
        assert np.array_equal(got[int(offsets[k]):int(offsets[k + 1])], tags[lo:hi]), (what, p)
        assert np.array_equal(u_got[int(u_offsets[k]):int(u_offsets[k + 1])], np.unique(tags[lo:hi])), (what, p)
    # the device form leaves the same rows in HBM
    csr_offsets, data = G.api._patterns_csr(patterns)
    t_off, p_off = guarded(csr_offsets, np.uint64, 8)
    t_dat, p_dat = guarded(data, np.uint8, 5)
    import torch
    torch.cuda.synchronize()
    for unique, (want_offsets, want_values) in ((False, (offsets, got)), (True, (u_offsets, u_got))):
        rows = fm.graph_positions_device(p_off, p_dat, len(patterns), data.size, unique=unique)
        assert rows.total == want_values.size and np.array_equal(view(rows.d_offsets, len(patterns) + 1), want_offsets) and np.array_equal(view(rows.d_values, rows.total), want_values)
    return fm, patterns


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_fixtures_graph_positions(name):
    dev = G.GBZ.load(os.path.join(O.GOLDEN, name))
    fm, _ = check_paths(dev, name)
    if name == "example.gbz":
        # by hand from example.gfa: G is the label of nodes 11 and 21; three paths go through each forward (P A and both W A; P B and both
        # W B), and the walk >21>22>24<23<21 ends on node 21 reversed, which reads C: so does node 16, on one path.  The 34 bytes of the
        # text are 6 endmarkers, 13 A, 2 C, 6 G and 7 T: the rows of C are [19, 21), those of G [21, 27)
        assert fm.count([b"G", b"C"])[:, 1].tolist() == [27, 21] and fm.count([b"G"]).tolist() == [[21, 27]]
        assert fm.graph_positions(b"G").tolist() == [11 << 11, 21 << 11]
        assert fm.graph_positions(b"G", unique=False).size == 6
        assert fm.graph_positions(b"C").tolist() == [16 << 11, (21 << 11) | (1 << 10)]
        assert fm.graph_positions(b"\0").tolist() == [0] and fm.graph_positions(b"\0", unique=False).tolist() == [0] * 6
    # refused: an index of a plain text, another handle, a workspace of another handle
    plain = G.FMIndex.from_text(b"GATTACA")
    offsets, data, out, total = np.array([0, 1], dtype=np.uint64), np.frombuffer(b"G", dtype=np.uint8), np.zeros(2, dtype=np.uint64), C.c_uint64(0)
    call = dev._L.gbwt_hip_fm_graph_positions
    assert call(plain._fm, dev._h, dev._ws, offsets.ctypes.data, data.ctypes.data, 1, 0, out.ctypes.data, None, 0, C.byref(total)) == _lib.BAD_ARGUMENT
    assert b"plain text" in dev._L.gbwt_hip_last_error()
    other = G.GBZ.load(os.path.join(O.GOLDEN, name))
    assert call(fm._fm, other._h, other._ws, offsets.ctypes.data, data.ctypes.data, 1, 0, out.ctypes.data, None, 0, C.byref(total)) == _lib.BAD_ARGUMENT
    assert b"another index handle" in dev._L.gbwt_hip_last_error()
    assert call(fm._fm, dev._h, other._ws, offsets.ctypes.data, data.ctypes.data, 1, 0, out.ctypes.data, None, 0, C.byref(total)) == _lib.BAD_ARGUMENT
    assert call(fm._fm, dev._h, dev._ws, offsets.ctypes.data, data.ctypes.data, 1, 2, out.ctypes.data, None, 0, C.byref(total)) == _lib.BAD_ARGUMENT
    assert call(fm._fm, dev._h, dev._ws, offsets.ctypes.data, data.ctypes.data, 1, 0, out.ctypes.data, None, 0, C.byref(total)) == _lib.OK
    with pytest.raises(ValueError):
        dev.fm_index([0], endmarker=None)
    lean = dev.fm_index(np.arange(dev.paths()), count_only=True)
    with pytest.raises(G.GbwtHipError) as e:
        lean.graph_positions_csr([b"G"])
    assert e.value.status == _lib.UNSUPPORTED
    for x in (plain, fm, lean):
        x.close()


def test_synthetic_genome_graph_positions(tmp_path):
    gbz = str(tmp_path / "genome.gbz")
    S.Synth.genome(contigs=2, fragments=2, haplotypes=8, sites=40, labels=1).save(gbz, as_gbz=True)
    dev = G.GBZ.load(gbz)
    fm, patterns = check_paths(dev, "synth")
    assert len(patterns) > 100
    # long rows are filled by whole waves: every single base occurs far more than 16 times
    assert (np.diff(fm.locate_csr([b"A", b"C", b"G", b"T"])[0].astype(np.int64)) > 64).all()
    fm.close()


def test_size_query_fill_protocol_and_memory():
    text = A.mutated_rows(4, 300, 3)
    patterns = [b"A", b"ACG", b"", b"ZZ", text[5:40]]
    offsets, data = G.api._patterns_csr(patterns)
    want_ranges, want_rows = expected(text, tuple(patterns))
    total_want = int((want_ranges[:, 1] - want_ranges[:, 0]).sum())
    fm = G.FMIndex.from_text(text)
    info = fm.info()
    # the plan's promise: the index the object keeps, and the scratch of the build, all of it gone
    assert info["index_bytes"] == info["planned_index_bytes"] == (len(text) + 1) // 96 * 128 + 128 + 1536 + 4 * len(text)
    assert info["peak_scratch_bytes"] == info["planned_scratch_bytes"] > 8 * len(text)
    assert info["queries"] == 0 and info["histogram_ms"] > 0 and info["codes_ms"] > 0 and info["counts_ms"] > 0 and info["fill_ms"] > 0 and info["narrow_ms"] > 0 and info["suffix_array_ms"] > 0
    L, total = fm._L, C.c_uint64(0)
    out_offsets = np.zeros(len(patterns) + 1, dtype=np.uint64)
    args = (fm._fm, offsets.ctypes.data, data.ctypes.data, len(patterns), out_offsets.ctypes.data)
    _lib.check(L.gbwt_hip_fm_locate(*args, None, 0, C.byref(total)))           # the size query computes
    sized = fm.info()
    assert total.value == total_want and sized["queries"] == 1 and sized["last_patterns"] == len(patterns) and sized["last_total"] == total_want
    assert sized["last_steps"] == 1 + 3 + 0 + 0 + 35 and sized["last_count_ms"] > 0
    positions = np.zeros(total_want, dtype=np.uint64)
    short = C.c_uint64(0)
    assert L.gbwt_hip_fm_locate(*args, positions.ctypes.data, total_want - 1, C.byref(short)) == _lib.CAPACITY and short.value == total_want
    assert str(total_want).encode() in L.gbwt_hip_last_error() and not positions.any()
    _lib.check(L.gbwt_hip_fm_locate(*args, positions.ctypes.data, total_want, C.byref(total)))      # the fill only copies
    assert fm.info() == sized
    assert np.array_equal(positions, np.concatenate(want_rows)) and np.array_equal(np.diff(out_offsets.astype(np.int64)), want_ranges[:, 1] - want_ranges[:, 0])
    # another request replaces the rows; a count in between as well
    fm.count(patterns)
    assert fm.info()["queries"] == 2 and fm.info()["last_total"] == 0
    _lib.check(L.gbwt_hip_fm_locate(*args, positions.ctypes.data, total_want, C.byref(total)))
    assert fm.info()["queries"] == 3
    fm.close()
