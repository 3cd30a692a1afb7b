"""The seeds of reads on the device (csrc/fm_seeds.hip, csrc/capi_fm_seeds.hip) against tests/seed_expect.py -- starts by `P[s:e] in text`,
the seed rule, ranges looked up in the brute-force suffix array -- at text level, and against the library's own tag_array of the true suffix
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
import seed_expect as E
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S
from test_gpu_tags import FIXTURES

pytestmark = pytest.mark.gpu

SMALL = A.small_texts()
GUARD = 0x5A


@functools.lru_cache(maxsize=None)
def stride():
    """K, read from the info of a request."""
    fm = G.FMIndex.from_text(b"ACGT", count_only=True)
    fm.seeds([b"A"])
    k = fm.last_seed_info()["stride"]
    fm.close()
    return k


@functools.lru_cache(maxsize=None)
def brute(text):
    sa = F.suffix_array(text)
    sa.setflags(write=False)
    return sa


@functools.lru_cache(maxsize=None)
def expected(text, read, strand):
    """All seeds of one strand of a read: computed once, shared by the sentinels, the options and the tests."""
    return tuple(E.expected(text, brute(text), read, strand))


@functools.lru_cache(maxsize=None)
def per_end_steps(text, read, strand):
    return E.per_end_steps(text, E.strand_read(read, strand))


def want_rows(text, reads, min_length, strands):
    return [[x for t in E.strands_of(strands) for x in expected(text, r, t) if x[1] - x[0] >= max(min_length, 1)] for r in reads]


def as_tuples(seeds):
    assert seeds.dtype == G.SEED_DTYPE and not seeds["reserved"].any()
    return list(zip(seeds["start"].tolist(), seeds["end"].tolist(), seeds["strand"].tolist(), seeds["lo"].tolist(), seeds["hi"].tolist()))


def rows_of(offsets, values):
    return [values[int(offsets[k]):int(offsets[k + 1])] for k in range(offsets.size - 1)]


def check_seeds(fm, text, reads, min_length, strands, what):
    read_offsets, seeds, hit_offsets, hits = fm.seeds(reads, min_length=min_length, strands=strands)
    assert hit_offsets is None and hits is None
    assert read_offsets.dtype == np.uint64 and read_offsets.size == len(reads) + 1 and read_offsets[0] == 0 and read_offsets[-1] == seeds.size, what
    got = as_tuples(seeds)
    for k, (read, want) in enumerate(zip(reads, want_rows(text, reads, min_length, strands))):
        assert got[int(read_offsets[k]):int(read_offsets[k + 1])] == want, (what, min_length, strands, k, read[:80])
    info = fm.last_seed_info()
    assert info["reads"] == len(reads) and info["read_bytes"] == sum(map(len, reads)) and info["strands"] == strands and info["seeds"] == seeds.size and info["hits"] == 0
    assert info["anchors"] == len(E.strands_of(strands)) * sum(-(-len(r) // info["stride"]) for r in reads)
    assert info["peak_scratch_bytes"] == info["planned_scratch_bytes"] > 0
    # never more backward steps than one search per end
    assert info["steps"] <= sum(per_end_steps(text, r, t) for r in reads for t in E.strands_of(strands)), what
    assert 0 <= info["idle_share"] < 1
    return info


@pytest.mark.parametrize("name,text", SMALL, ids=[name for name, _ in SMALL])
def test_small_texts_against_the_yardstick(name, text):
    K = stride()
    reads = E.reads_of(text, K)
    lengths = [len(r) for r in reads]
    assert len(reads) % 64 != 0 and lengths[:7] == [0, 1, K - 1, K, K + 1, 2 * K + 1, 77] and reads[-1] == text
    if len(set(text)) < 256:                                                   # a byte the text lacks: first, middle, last, and nothing else
        lack = reads[-2][0]
        assert lack not in text and reads[-2] == bytes([lack]) * 5 and [r.index(lack) for r in reads[-5:-2]] == [0, K, 2 * K]
        assert want_rows(text, [reads[-2]], 1, E.FORWARD) == [[]]
    for sentinel in (0, 65, 255):
        fm = G.FMIndex.from_text(text, sentinel=sentinel)
        for min_length in (1, 5):
            for strands in (G.STRAND_FORWARD, G.STRAND_REVERSE, G.STRAND_BOTH):
                check_seeds(fm, text, reads, min_length, strands, (name, sentinel))
        empty = fm.seeds([])
        assert empty[0].tolist() == [0] and empty[1].size == 0 and fm.last_seed_info()["anchors"] == 0
        assert fm.seeds([b"", b""])[0].tolist() == [0, 0, 0]
        fm.close()


def test_a_run_refines_the_last_interval_only():
    K = stride()
    text = dict(SMALL)["a_run"]
    assert text == b"A" * 5000 + b"\0"
    fm = G.FMIndex.from_text(text)
    read = b"A" * 5001
    read_offsets, seeds, _, _ = fm.seeds([read], strands=G.STRAND_FORWARD)
    lo = int(np.flatnonzero(brute(text) == 0)[0])
    assert as_tuples(seeds) == [(0, 5000, 1, lo, lo + 1), (1, 5001, 1, lo, lo + 1)] == want_rows(text, [read], 1, E.FORWARD)[0] and read_offsets.tolist() == [0, 2]
    info = fm.last_seed_info()
    assert info["refined_ends"] == K - 1 and info["anchors"] == -(-5001 // K) and info["stride"] == K
    fm.close()


@pytest.mark.parametrize("letters", [b"ACGT", b"ACGTNRYKMSWB"], ids=["packed", "plain"])
def test_block_edges(letters):
    rng = np.random.default_rng(23)
    alphabet = np.frombuffer(letters, dtype=np.uint8)
    B = 96 if len(letters) <= 8 else 256
    for n in (B - 1, B, B + 1, 2 * B, 2 * B + 1):
        text = alphabet[rng.integers(0, alphabet.size, size=n)].tobytes()
        fm = G.FMIndex.from_text(text, sentinel=65)
        assert fm.info()["block_rows"] == B and fm.info()["blocks"] == (n + 1) // B + 1
        check_seeds(fm, text, E.reads_of(text, stride(), rounds=3), 1, G.STRAND_BOTH, (letters, n))
        fm.close()


def test_strand_identity():
    text = A.mutated_rows(4, 300, 3)
    rng = np.random.default_rng(37)
    reads = []
    for r in E.reads_of(text[:900], stride(), rounds=4):
        r = bytearray(r)
        for at in rng.integers(0, max(len(r), 1), size=len(r) // 9):
            r[at] = rng.choice(np.frombuffer(b"acgtNn\0", dtype=np.uint8))
        reads.append(bytes(r))
    assert any(b"a" in r for r in reads) and any(b"N" in r for r in reads)
    fm = G.FMIndex.from_text(text)
    for min_length in (1, 5):
        r_offsets, r_seeds, _, _ = fm.seeds(reads, min_length=min_length, strands=G.STRAND_REVERSE)
        f_offsets, f_seeds, _, _ = fm.seeds([G.reverse_complement(r) for r in reads], min_length=min_length, strands=G.STRAND_FORWARD)
        assert np.array_equal(r_offsets, f_offsets) and r_seeds.size == f_seeds.size > 0
        assert (r_seeds["strand"] == G.STRAND_REVERSE).all() and (f_seeds["strand"] == G.STRAND_FORWARD).all()
        for field in ("lo", "hi", "start", "end"):
            assert np.array_equal(r_seeds[field], f_seeds[field]), field
    # no case folding on the forward strand; the reverse strand folds
    assert fm.seeds([b"acgt"], strands=G.STRAND_FORWARD)[1].size == 0 and fm.seeds([b"acgt"], strands=G.STRAND_REVERSE)[1].size > 0
    # a read's row: its forward seeds, then its reverse seeds
    both = fm.seeds(reads, strands=G.STRAND_BOTH)
    for row in rows_of(both[0], both[1]):
        strands = row["strand"].tolist()
        assert strands == sorted(strands)
        for t in (1, 2):
            one = row[row["strand"] == t]
            assert (np.diff(one["start"].astype(np.int64)) > 0).all() and (np.diff(one["end"].astype(np.int64)) > 0).all()
    check_seeds(fm, text, reads, 1, G.STRAND_BOTH, "strand identity")
    fm.close()


def check_hits(fm, sa, reads, max_occurrences, values=None, **more):
    """Row i of the hits is values[lo:hi] (the suffix array, or what stands for it) where the seed has at most max_occurrences, else empty."""
    values = sa if values is None else values
    read_offsets, seeds, hit_offsets, hits = fm.seeds(reads, max_occurrences=max_occurrences, **more)
    assert hit_offsets.size == seeds.size + 1 and hit_offsets[0] == 0 and hit_offsets[-1] == hits.size
    over = 0
    for seed, row in zip(seeds, rows_of(hit_offsets, hits)):
        lo, hi = int(seed["lo"]), int(seed["hi"])
        if hi - lo <= max_occurrences:
            assert np.array_equal(row, values[lo:hi]), (seed, max_occurrences)
        else:
            assert row.size == 0
            over += 1
    info = fm.last_seed_info()
    assert info["hits"] == hits.size and info["over_max"] == over and info["seeds"] == seeds.size
    return seeds, over


def test_hits():
    text = A.mutated_rows(4, 300, 3)
    sa = brute(text).astype(np.uint64)
    reads = E.reads_of(text[:900], stride(), rounds=4) + [text[10:160]]
    fm = G.FMIndex.from_text(text)
    seeds, over = check_hits(fm, sa, reads, 1 << 20)
    assert over == 0 and as_tuples(seeds) == [x for row in want_rows(text, reads, 1, E.BOTH) for x in row]
    counts = (seeds["hi"] - seeds["lo"]).astype(np.int64)
    c = int(counts[counts > 1].min())                                          # at, below and above a seed's count
    for most, none_over in ((c, False), (c - 1, True), (c + 1, False)):
        again, over = check_hits(fm, sa, reads, most)
        assert np.array_equal(again, seeds) and over == int((counts > most).sum()) and (over > 0 or not none_over)
    fm.close()
    # long rows are filled by whole waves
    text = dict(SMALL)["ac"]
    fm = G.FMIndex.from_text(text)
    seeds, over = check_hits(fm, brute(text).astype(np.uint64), [b"ACAC", b"CACACAT"], 5000, strands=G.STRAND_FORWARD)
    assert over == 0 and as_tuples(seeds)[0][:2] == (0, 4) and as_tuples(seeds)[1][:2] == (0, 6) and (seeds["hi"] - seeds["lo"]).tolist() == [2499, 2497]
    fm.close()
    # a count-only index finds seeds and refuses hits
    lean = G.FMIndex.from_text(A.mutated_rows(4, 300, 3), count_only=True)
    check_seeds(lean, A.mutated_rows(4, 300, 3), reads, 1, G.STRAND_BOTH, "count-only")
    with pytest.raises(G.GbwtHipError) as e:
        lean.seeds(reads, max_occurrences=5)
    assert e.value.status == _lib.UNSUPPORTED
    lean.close()


def path_reads(text, rng):
    """Reads cut from the text of the paths -- some with a base replaced --, and their reverse complements."""
    reads = []
    for length in (1, 5, 16, 17, 33, 60):
        for _ in range(4):
            if len(text) < length:
                continue
            at = int(rng.integers(0, len(text) - length + 1))
            r = bytearray(text[at:at + length])
            if length > 16 and rng.integers(0, 2):
                r[length // 2] = ord("ACGT"[int(rng.integers(0, 4))])
            reads.append(bytes(r))
    return reads + [G.reverse_complement(r) for r in reads]


def check_paths(dev, what):
    ids = np.arange(dev.paths(), dtype=np.uint64)
    _, text = dev.path_sequences(ids, endmarker=0)
    text = bytes(text)
    sa = brute(text)
    tags = dev.tag_array(ids, sa)
    reads = path_reads(text, np.random.default_rng(43))
    fm = dev.fm_index(ids)
    check_seeds(fm, text, reads, 1, G.STRAND_BOTH, what)
    check_hits(fm, sa.astype(np.uint64), reads, 1 << 20)
    for most in (1 << 20, 2):
        seeds, _ = check_hits(fm, sa, reads, most, values=tags, graph=True)
        assert as_tuples(seeds) == [x for row in want_rows(text, reads, 1, E.BOTH) for x in row], what
    return fm, reads


def guarded(array, lead):
    """`array` in device memory with `lead` guard bytes in front and 16 behind: (tensor, device pointer of the payload)."""
    import torch
    raw = np.concatenate([np.full(lead, GUARD, np.uint8), np.ascontiguousarray(array).view(np.uint8).reshape(-1), np.full(16, GUARD, np.uint8)])
    t = torch.from_numpy(raw).to("cuda:0")
    return t, t.data_ptr() + lead


def view(pointer, count):
    import torch
    from gbwt_rs_amd import dist as D
    if count == 0:
        return np.zeros(0, dtype=np.uint64)
    return D.device_view(pointer, count * 8, torch.uint8, torch.device("cuda:0")).cpu().numpy().view(np.uint64).copy()


def check_device_form(fm, reads, host, **more):
    """The device form leaves the rows of the host form in HBM and the caller's buffers as they were."""
    import torch
    offsets, data = G.api._patterns_csr(reads)
    t_off, p_off = guarded(offsets, 8)
    t_dat, p_dat = guarded(data, 3)
    torch.cuda.synchronize()
    rows = fm.seeds_device(p_off, p_dat, len(reads), data.size, **more)
    h_offsets, h_seeds, h_hit_offsets, h_hits = host
    assert rows.m == len(reads) and rows.total_seeds == h_seeds.size and np.array_equal(view(rows.d_read_offsets, len(reads) + 1), h_offsets)
    assert np.array_equal(view(rows.d_seeds, 4 * rows.total_seeds).view(G.SEED_DTYPE), h_seeds)
    if h_hits is None:
        assert rows.d_hit_offsets is None and rows.d_hits is None and rows.total_hits == 0
    else:
        assert rows.total_hits == h_hits.size and np.array_equal(view(rows.d_hit_offsets, rows.total_seeds + 1), h_hit_offsets) and np.array_equal(view(rows.d_hits, rows.total_hits), h_hits)
    # offsets that leave the read bytes are found by the kernel
    with pytest.raises(G.GbwtHipError) as e:
        fm.seeds_device(p_off, p_dat, len(reads), data.size - 1, **more)
    assert e.value.status == _lib.BAD_ARGUMENT and "leave the pattern bytes" in str(e.value)
    for t, lead, payload in ((t_off, 8, 8 * (len(reads) + 1)), (t_dat, 3, data.size)):
        raw = t.cpu().numpy()
        assert (raw[:lead] == GUARD).all() and (raw[lead + payload:] == GUARD).all() and raw.size == lead + payload + 16
    assert np.array_equal(t_off.cpu().numpy()[8:-16].view(np.uint64), offsets) and np.array_equal(t_dat.cpu().numpy()[3:-16], data)


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_fixtures_seed_graph_positions(name):
    dev = G.GBZ.load(os.path.join(O.GOLDEN, name))
    fm, reads = check_paths(dev, name)
    check_device_form(fm, reads, fm.seeds(reads, max_occurrences=50, graph=True), max_occurrences=50, graph=True)
    # refused: no hits asked for, an index of a plain text, another handle, a workspace of another handle
    plain = G.FMIndex.from_text(b"GATTACA")
    offsets, data = G.api._patterns_csr([b"G"])
    out, n_seeds, n_hits, opts = np.zeros(2, dtype=np.uint64), C.c_uint64(0), C.c_uint64(0), _lib.FmSeedOptions(1, 3, 5, 0, 0)
    call = dev._L.gbwt_hip_fm_seed_graph_positions

    def ask(fm_, h, ws, options=opts):
        return call(fm_, h, ws, offsets.ctypes.data, data.ctypes.data, 1, C.byref(options), out.ctypes.data, None, 0, C.byref(n_seeds), None, None, 0, C.byref(n_hits))
    assert ask(fm._fm, dev._h, dev._ws, _lib.FmSeedOptions(1, 3, 0, 0, 0)) == _lib.BAD_ARGUMENT and b"max_occurrences > 0" in dev._L.gbwt_hip_last_error()
    assert ask(plain._fm, dev._h, dev._ws) == _lib.BAD_ARGUMENT and b"plain text" in dev._L.gbwt_hip_last_error()
    other = G.GBZ.load(os.path.join(O.GOLDEN, name))
    assert ask(fm._fm, other._h, other._ws) == _lib.BAD_ARGUMENT and b"another index handle" in dev._L.gbwt_hip_last_error()
    assert ask(fm._fm, dev._h, other._ws) == _lib.BAD_ARGUMENT and b"mismatched" in dev._L.gbwt_hip_last_error()
    assert ask(fm._fm, dev._h, dev._ws) == _lib.OK and n_seeds.value > 0
    lean = dev.fm_index(np.arange(dev.paths()), count_only=True)
    with pytest.raises(G.GbwtHipError) as e:
        lean.seeds([b"G"], max_occurrences=5, graph=True)
    assert e.value.status == _lib.UNSUPPORTED
    assert lean.seeds(reads[:1])[1].size > 0
    for x in (plain, fm, lean):
        x.close()


def test_synthetic_genome_seed_graph_positions(tmp_path):
    gbz = str(tmp_path / "genome.gbz")
    S.Synth.genome(contigs=2, fragments=2, haplotypes=8, sites=40, labels=1).save(gbz, as_gbz=True)
    dev = G.GBZ.load(gbz)
    fm, reads = check_paths(dev, "synth")
    assert len(reads) >= 40
    fm.close()


def test_device_forms():
    text = A.mutated_rows(4, 300, 3) + b"ACGTTGCA"
    reads = E.reads_of(text[:900], stride(), rounds=4)
    fm = G.FMIndex.from_text(text)
    for more in (dict(), dict(min_length=5, strands=G.STRAND_REVERSE), dict(max_occurrences=3), dict(max_occurrences=1 << 20, strands=G.STRAND_FORWARD)):
        check_device_form(fm, reads, fm.seeds(reads, **more), **more)
    fm.close()


def test_size_query_fill_protocol_and_scratch():
    text = A.mutated_rows(4, 300, 3)
    reads = [b"A", text[5:40], b"", b"ZZ", text[100:130] + b"T" + text[131:170], b"ACGT" * 3]
    offsets, data = G.api._patterns_csr(reads)
    want = [x for row in want_rows(text, reads, 1, E.BOTH) for x in row]
    sa = brute(text).astype(np.uint64)
    fm = G.FMIndex.from_text(text)
    assert fm.last_seed_info()["requests"] == 0
    L, n_seeds, n_hits = fm._L, C.c_uint64(0), C.c_uint64(0)
    opts = _lib.FmSeedOptions(1, 3, 1 << 20, 0, 0)
    read_offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    args = (fm._fm, offsets.ctypes.data, data.ctypes.data, len(reads), C.byref(opts), read_offsets.ctypes.data)
    _lib.check(L.gbwt_hip_fm_seeds(*args, None, 0, C.byref(n_seeds), None, None, 0, C.byref(n_hits)))       # the size query computes
    sized = fm.last_seed_info()
    total_hits = sum(hi - lo for _, _, _, lo, hi in want)
    assert n_seeds.value == len(want) and n_hits.value == total_hits and sized["requests"] == 1 and sized["seeds"] == len(want) and sized["hits"] == total_hits
    assert sized["peak_scratch_bytes"] == sized["planned_scratch_bytes"] > 0 and sized["anchor_ms"] > 0 and sized["emit_ms"] > 0 and sized["hits_ms"] > 0 and sized["steps"] > 0
    assert read_offsets[-1] == len(want)
    seeds, hit_offsets, hits = np.zeros(len(want), dtype=G.SEED_DTYPE), np.zeros(len(want) + 1, dtype=np.uint64), np.zeros(total_hits, dtype=np.uint64)
    # a capacity that is too small: the totals, and nothing written
    read_offsets[:] = 77
    for seed_capacity, hit_capacity, word in ((len(want) - 1, total_hits, b"seed capacity"), (len(want), total_hits - 1, b"hit capacity")):
        a, b = C.c_uint64(0), C.c_uint64(0)
        status = L.gbwt_hip_fm_seeds(*args, seeds.ctypes.data, seed_capacity, C.byref(a), hit_offsets.ctypes.data, hits.ctypes.data, hit_capacity, C.byref(b))
        assert status == _lib.CAPACITY and (a.value, b.value) == (len(want), total_hits) and word in L.gbwt_hip_last_error()
        assert not seeds.view(np.uint8).any() and not hit_offsets.any() and not hits.any() and (read_offsets == 77).all()
    _lib.check(L.gbwt_hip_fm_seeds(*args, seeds.ctypes.data, len(want), C.byref(n_seeds), hit_offsets.ctypes.data, hits.ctypes.data, total_hits, C.byref(n_hits)))   # the fill only copies
    assert fm.last_seed_info() == sized
    assert as_tuples(seeds) == want and hit_offsets[-1] == total_hits
    for (_, _, _, lo, hi), row in zip(want, rows_of(hit_offsets, hits)):
        assert np.array_equal(row, sa[lo:hi])
    # other options are another request; the queries beside it keep their own rows
    fm.seeds(reads, min_length=5)
    assert fm.last_seed_info()["requests"] == 2 and fm.last_seed_info()["hits"] == 0
    located = fm.locate_csr([b"ACG"])
    fm.seeds(reads, min_length=5)
    assert fm.last_seed_info()["requests"] == 2 and fm.info()["queries"] == 1
    assert np.array_equal(fm.locate_csr([b"ACG"])[1], located[1]) and fm.info()["queries"] == 1
    fm.close()


def test_counted_promise_of_the_plan():
    """A condition, not a timing: reads cut from the text cost their anchors and nothing else."""
    K = stride()
    text = A.mutated_rows(3, 400, 2, seed=9)
    row = text[:400]
    lengths = [150, 150, 77, K, K + 1, 2 * K + 1, 1, 0, 399, 400]
    reads = [row[at:at + n] for at, n in zip(range(0, 400, 7), lengths) if at + n <= 400] + [row]
    assert len(reads) >= 9 and all(r in text for r in reads)
    fm = G.FMIndex.from_text(text)
    info = check_seeds(fm, text, reads, 1, G.STRAND_FORWARD, "cut from the text")
    assert info["stride"] == K and info["refined_ends"] == 0
    assert info["steps"] == sum(len(r) - j * K for r in reads for j in range(-(-len(r) // K))) == sum(E.anchored_steps_of_matching_read(len(r), K) for r in reads)
    assert info["seeds"] == sum(1 for r in reads if r)
    fm.close()
