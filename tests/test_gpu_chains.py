"""The chains of seeds on the device (csrc/fm_chains.hip, csrc/capi_fm_chains.hip) against tests/chain_expect.py -- the definition in numpy over
the seeds of tests/seed_expect.py and the brute-force suffix array --, field for field, at the smallest shapes where each piece can go wrong."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import chain_expect as X
import fm_expect as F
import gbwt_rs_amd as G
import oracle_lib as O
import sa_expect as A
import seed_expect as E
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S
from test_chains_cpu import SETTINGS, case_reads, replaced
from test_gpu_seeds import GUARD, guarded, path_reads, view

pytestmark = pytest.mark.gpu

MOST = 1 << 20


@functools.lru_cache(maxsize=None)
def brute(text):
    sa = F.suffix_array(text)
    sa.setflags(write=False)
    return sa


def chain_tuples(chains):
    assert chains.dtype == G.CHAIN_DTYPE
    return list(zip(*(chains[name].tolist() for name in G.CHAIN_DTYPE.names)))


def match_tuples(matches):
    assert matches.dtype == G.CHAIN_MATCH_DTYPE
    return list(zip(matches["y"].tolist(), matches["x"].tolist(), matches["w"].tolist()))


def check(fm, text, reads, bounds=None, **options):
    """One request against the yardstick: every output field, and the counts of the info."""
    want = X.expected_rows(text, brute(text), reads, bounds=bounds, **options)
    read_offsets, chains, match_offsets, matches = fm.chains(reads, **options)
    assert read_offsets.dtype == match_offsets.dtype == np.uint64
    assert read_offsets.tolist() == want["read_offsets"], options
    assert chain_tuples(chains) == want["chains"], options
    assert match_offsets.tolist() == want["match_offsets"], options
    assert match_tuples(matches) == want["matches"], options
    info = fm.last_chain_info()
    assert (info["items"], info["matches"], info["pairs"], info["chains"], info["chain_matches"], info["skipped_items"]) == \
        (want["items"], want["n_matches"], want["pairs"], len(want["chains"]), len(want["matches"]), want["skipped_items"]), options
    assert info["planned_scratch_bytes"] == info["peak_scratch_bytes"] > 0
    assert info["path_offset_bytes"] == (0 if bounds is None else max(8 * len(bounds), 256))
    return want, info


def rows_of_read(want, k):
    return want["chains"][want["read_offsets"][k]:want["read_offsets"][k + 1]]


def test_substitutions_indels_junk_and_empties():
    text = A.mutated_rows(4, 300, 3)
    reads = case_reads(text)
    assert reads[6:] == [b"", b"A", b"ZZZ"] and len(reads[2]) == 147 and len(reads[3]) == 155
    fm = G.FMIndex.from_text(text)
    for max_gap, max_skew, gap_cost, min_score in SETTINGS:
        want, _ = check(fm, text, reads, min_length=5, strands=G.STRAND_BOTH, max_occurrences=MOST, max_gap=max_gap, max_skew=max_skew, gap_cost=gap_cost, min_score=min_score)
        forward = [[row for row in rows_of_read(want, k) if row[6] == E.FORWARD] for k in range(len(reads))]
        joined = [row for row in forward[4] if row[5] >= 2 and row[2] < 40 and row[3] > 80]
        if (max_gap, max_skew, gap_cost, min_score) == (1000, 50, 1, 1):
            assert [forward[k][0][4:6] for k in range(4)] == [(150, 1), (131, 3), (137, 2), (135, 2)]
            assert not joined                                                     # the two pieces: skew 140 > 50
            assert any(len(rows_of_read(want, k)) > 2 for k in range(6))
        if gap_cost == 0:
            assert max_skew >= 140 and joined and joined[0][4:6] == (108, 2)
        if min_score == 20:
            assert all(row[4] >= 20 for row in want["chains"]) and len(want["chains"]) < 20
        assert want["read_offsets"][6:] == [want["read_offsets"][6]] * 4
    fm.close()


def test_equal_chains():
    text = A.mutated_rows(4, 300, 0)
    fm = G.FMIndex.from_text(text)
    want, _ = check(fm, text, [replaced(text[20:170])], min_length=5, strands=G.STRAND_FORWARD, max_occurrences=MOST, max_gap=1000, max_skew=50)
    assert [row[4:6] for row in want["chains"][:4]] == [(131, 3)] * 4 and [row[0] for row in want["chains"][:4]] == [20, 321, 622, 923]
    assert len(want["chains"]) > 4 and all(row[5] == 1 for row in want["chains"][4:])
    fm.close()


def check_segments(dev, what):
    ids = np.arange(dev.paths(), dtype=np.uint64)
    offsets, text = dev.path_sequences(ids, endmarker=0)
    text, bounds = bytes(text), [int(v) for v in offsets]
    assert bounds[0] == 0 and bounds[-1] == len(text) and all(text[b - 1] == 0 for b in bounds[1:])     # the cumulated len + 1 of the path texts
    across = []
    for k in range(1, len(bounds) - 1):                                           # the last bases of a path and the first of the next, without the endmarker
        head, tail = min(30, bounds[k] - 1 - bounds[k - 1]), min(30, bounds[k + 1] - 1 - bounds[k])
        across.append(text[bounds[k] - 1 - head:bounds[k] - 1] + text[bounds[k]:bounds[k] + tail])
    across = across[:6]
    reads = across + path_reads(text, np.random.default_rng(43))[:24]
    assert across and all(0 not in r for r in across)
    fm = dev.fm_index(ids)
    options = dict(min_length=4, strands=G.STRAND_BOTH, max_occurrences=MOST, max_gap=1000, max_skew=50)
    want, info = check(fm, text, reads, bounds=bounds, **options)
    assert info["path_offset_bytes"] >= 8 * len(bounds) and want["chains"]
    for at, row in enumerate(want["chains"]):                                     # `path` names the path a chain starts in, and a chain of a read without
        assert bounds[row[7]] <= row[0] < bounds[row[7] + 1], (what, row)         # an endmarker does not leave it
        assert at >= want["read_offsets"][len(across)] or row[1] <= bounds[row[7] + 1] - 1, (what, row)
    assert len({row[7] for row in want["chains"]}) > 1
    fm.close()
    plain = G.FMIndex.from_text(text)                                             # the same bytes as a plain text do join
    joined, _ = check(plain, text, reads, **options)
    crossing = [row for row in joined["chains"] if any(row[0] < b <= row[1] - 1 for b in bounds[1:-1])]
    assert crossing and all(row[7] == 0 for row in joined["chains"]), what
    assert joined["chains"] != want["chains"]
    plain.close()


def test_segments_of_a_golden_fixture():
    check_segments(G.GBZ.load(os.path.join(O.GOLDEN, "example.gbz")), "example.gbz")


def test_segments_of_a_synthetic_genome(tmp_path):
    gbz = str(tmp_path / "genome.gbz")
    S.Synth.genome(contigs=2, fragments=2, haplotypes=8, sites=40, labels=1).save(gbz, as_gbz=True)
    check_segments(G.GBZ.load(gbz), "synth")


def test_segments_on_rows_of_a_text():
    """The figures of the definition: 99 from 2 matches without bounds against 60 with them."""
    text = A.mutated_rows(4, 300, 3)
    across = [text[240:300] + text[301:341]]
    want = X.expected_rows(text, brute(text), across, 5, E.FORWARD, MOST, 1000, 50, 1, 1)
    cut = X.expected_rows(text, brute(text), across, 5, E.FORWARD, MOST, 1000, 50, 1, 1, bounds=[0, 301, 602, 903, 1204])
    assert want["chains"][0][4:6] == (99, 2) and cut["chains"][0][4:6] == (60, 1)
    fm = G.FMIndex.from_text(text)
    check(fm, text, across, min_length=5, strands=G.STRAND_FORWARD, max_occurrences=MOST, max_gap=1000, max_skew=50)
    fm.close()


def test_windows_wider_than_a_wave_and_items_larger_than_the_tile():
    probe = G.FMIndex.from_text(b"ACGT")
    tile = probe.last_chain_info()["tile_matches"]
    probe.close()
    assert 64 <= tile <= 4096
    read = b"ACACAC" + b"G" + b"ACACAC"
    options = dict(min_length=5, strands=G.STRAND_FORWARD, max_occurrences=MOST, max_gap=400, max_skew=8)
    for reps in (tile // 2 + 3, 40):
        text = b"AC" * reps + b"\0"
        fm = G.FMIndex.from_text(text)
        want, info = check(fm, text, [read], **options)
        count = 2 * (reps - 2)                                                    # ACACAC at x = 0 and at x = 7, each at every even y
        assert info["matches"] == count and (count >= tile + 1) == (reps != 40)
        assert min(count, 400) > 64                                               # the window of an i: two matches at every even y of the 400 in front, some 100 at reps = 40
        assert want["chains"][0][4:6] == (11, 2) and info["pairs"] > count        # dy 6 and dy 8 both give 6 + 6 - 1: the larger j wins
        # one below the item's count: no chains, and the item is counted
        skipped, _ = check(fm, text, [read], max_matches=count - 1, **options)
        assert skipped["skipped_items"] == 1 and skipped["chains"] == [] and skipped["read_offsets"] == [0, 0]
        check(fm, text, [read], max_matches=count, **options)
        fm.close()


@pytest.mark.parametrize("reads_in_batch", [63, 64, 65, 129])
def test_batch_edges(reads_in_batch):
    text = A.mutated_rows(1, 600, 0, seed=11) + A.mutated_rows(2, 120, 1, seed=12)
    rng = np.random.default_rng(reads_in_batch)
    reads = []
    for k in range(reads_in_batch):
        kind = k % 4
        at = int(rng.integers(0, 570))
        reads.append(b"" if kind == 0 else b"ZZZ" if kind == 1 and k % 8 == 1 else text[at:at + 21] if kind < 3 else replaced(text[620:720], (30, 60)))
    fm = G.FMIndex.from_text(text)
    options = dict(min_length=5, max_occurrences=MOST, max_gap=1000, max_skew=50)
    want, info = check(fm, text, reads, strands=G.STRAND_FORWARD, **options)
    sizes = [want["read_offsets"][k + 1] - want["read_offsets"][k] for k in range(reads_in_batch)]
    assert 0 in sizes and 1 in sizes and max(sizes) > 1 and info["items"] == reads_in_batch
    # the seeds' strand identity: the reverse strand of a read is the forward strand of its reverse complement
    reverse = fm.chains(reads, strands=G.STRAND_REVERSE, **options)
    forward = fm.chains([G.reverse_complement(r) for r in reads], strands=G.STRAND_FORWARD, **options)
    assert np.array_equal(reverse[0], forward[0]) and np.array_equal(reverse[2], forward[2]) and np.array_equal(reverse[3], forward[3]) and reverse[1].size > 0
    assert (reverse[1]["strand"] == G.STRAND_REVERSE).all() and (forward[1]["strand"] == G.STRAND_FORWARD).all()
    for name in G.CHAIN_DTYPE.names:
        assert name == "strand" or np.array_equal(reverse[1][name], forward[1][name]), name
    check(fm, text, reads, strands=G.STRAND_REVERSE, **options)
    if reads_in_batch == 65:
        check(fm, text, reads, strands=G.STRAND_BOTH, **options)
    fm.close()


def test_size_query_fill_protocol_and_requests():
    text = A.mutated_rows(4, 300, 3)
    reads = case_reads(text)
    offsets, data = G.api._patterns_csr(reads)
    want = X.expected_rows(text, brute(text), reads, 5, E.BOTH, MOST, 1000, 50, 1, 1)
    n_c, n_m = len(want["chains"]), len(want["matches"])
    fm = G.FMIndex.from_text(text)
    assert fm.last_chain_info()["requests"] == 0
    L, total_chains, total_matches = fm._L, C.c_uint64(0), C.c_uint64(0)
    seed_opts, chain_opts = _lib.FmSeedOptions(5, 3, MOST, 0, 0), _lib.FmChainOptions(1000, 50, 1, 1, 0, 0, 0)
    read_offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    args = (fm._fm, offsets.ctypes.data, data.ctypes.data, len(reads), C.byref(seed_opts), C.byref(chain_opts), read_offsets.ctypes.data)
    _lib.check(L.gbwt_hip_fm_chains(*args, None, 0, C.byref(total_chains), None, None, 0, C.byref(total_matches)))      # the size query computes
    sized = fm.last_chain_info()
    assert (total_chains.value, total_matches.value) == (n_c, n_m) and sized["requests"] == 1 and sized["chains"] == n_c and read_offsets.tolist() == want["read_offsets"]
    assert sized["seeds_ms"] > 0 and sized["expand_ms"] > 0 and sized["sort_ms"] > 0 and sized["dp_ms"] > 0 and sized["peel_ms"] > 0 and sized["fill_ms"] > 0
    assert fm.last_seed_info()["requests"] == 1 and fm.last_seed_info()["hits"] == want["n_matches"]
    chains, match_offsets, matches = np.zeros(n_c, dtype=G.CHAIN_DTYPE), np.zeros(n_c + 1, dtype=np.uint64), np.zeros(n_m, dtype=G.CHAIN_MATCH_DTYPE)
    # a capacity that is too small: the totals, and nothing written
    read_offsets[:] = 77
    for chain_capacity, match_capacity, word in ((n_c - 1, n_m, b"chain capacity"), (n_c, n_m - 1, b"match capacity")):
        a, b = C.c_uint64(0), C.c_uint64(0)
        status = L.gbwt_hip_fm_chains(*args, chains.ctypes.data, chain_capacity, C.byref(a), match_offsets.ctypes.data, matches.ctypes.data, match_capacity, C.byref(b))
        assert status == _lib.CAPACITY and (a.value, b.value) == (n_c, n_m) and word in L.gbwt_hip_last_error()
        assert not chains.view(np.uint8).any() and not match_offsets.any() and not matches.view(np.uint8).any() and (read_offsets == 77).all()
    _lib.check(L.gbwt_hip_fm_chains(*args, chains.ctypes.data, n_c, C.byref(total_chains), match_offsets.ctypes.data, matches.ctypes.data, n_m, C.byref(total_matches)))   # the fill only copies
    assert fm.last_chain_info() == sized
    assert chain_tuples(chains) == want["chains"] and match_offsets.tolist() == want["match_offsets"] and match_tuples(matches) == want["matches"]
    # a seeds call with the same arguments computes nothing: the seeds rows are those of the chains request
    seeds = fm.seeds(reads, min_length=5, strands=G.STRAND_BOTH, max_occurrences=MOST)
    assert fm.last_seed_info()["requests"] == 1 and seeds[3].size == want["n_matches"]
    # other chain options are another request, on the same seeds
    check(fm, text, reads, min_length=5, strands=G.STRAND_BOTH, max_occurrences=MOST, max_gap=1000, max_skew=2)
    again = fm.last_chain_info()
    assert again["requests"] == 2 and again["seeds_ms"] == 0 and fm.last_seed_info()["requests"] == 1
    fm.chains(reads, min_length=5, strands=G.STRAND_BOTH, max_occurrences=MOST, max_gap=1000, max_skew=2)
    assert fm.last_chain_info() == again
    # the device form: the rows of the host form in HBM, the caller's buffers as they were
    import torch
    host = fm.chains(reads, min_length=5, max_occurrences=MOST, max_gap=100, max_skew=10, gap_cost=2, min_score=20)
    t_off, p_off = guarded(offsets, 8)
    t_dat, p_dat = guarded(data, 3)
    torch.cuda.synchronize()
    rows = fm.chains_device(p_off, p_dat, len(reads), data.size, min_length=5, max_occurrences=MOST, max_gap=100, max_skew=10, gap_cost=2, min_score=20)
    assert rows.m == len(reads) and rows.total_chains == host[1].size > 0 and rows.total_matches == host[3].size
    assert np.array_equal(view(rows.d_read_offsets, len(reads) + 1), host[0]) and np.array_equal(view(rows.d_match_offsets, rows.total_chains + 1), host[2])
    assert np.array_equal(view(rows.d_chains, 5 * rows.total_chains).view(G.CHAIN_DTYPE), host[1])
    assert np.array_equal(view(rows.d_matches, 2 * rows.total_matches).view(G.CHAIN_MATCH_DTYPE), host[3])
    with pytest.raises(G.GbwtHipError) as e:
        fm.chains_device(p_off, p_dat, len(reads), data.size - 1, min_length=5, max_occurrences=MOST)
    assert e.value.status == _lib.BAD_ARGUMENT and "leave the pattern bytes" in str(e.value)
    for t, lead, payload in ((t_off, 8, 8 * (len(reads) + 1)), (t_dat, 3, data.size)):
        raw = t.cpu().numpy()
        assert (raw[:lead] == GUARD).all() and (raw[lead + payload:] == GUARD).all() and raw.size == lead + payload + 16
    assert np.array_equal(t_off.cpu().numpy()[8:-16].view(np.uint64), offsets) and np.array_equal(t_dat.cpu().numpy()[3:-16], data)
    # no reads, and reads without a seed
    assert [a.tolist() for a in fm.chains([], max_occurrences=5)] == [[0], [], [0], []]
    assert fm.chains([b"", b"ZZ"], max_occurrences=5)[0].tolist() == [0, 0, 0]
    fm.close()
    # a count-only index holds no hits to chain; chains need hits
    lean = G.FMIndex.from_text(text, count_only=True)
    with pytest.raises(G.GbwtHipError) as e:
        lean.chains(reads, max_occurrences=5)
    assert e.value.status == _lib.UNSUPPORTED
    with pytest.raises(G.GbwtHipError) as e:
        lean.chains(reads, max_occurrences=0)
    assert e.value.status == _lib.BAD_ARGUMENT and "chains need hits" in str(e.value)
    lean.close()
