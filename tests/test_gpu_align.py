"""The alignments of chains on the device (csrc/fm_align.hip, csrc/capi_fm_align.hip) against tests/align_expect.py -- the definition in plain
loops over the chains of tests/chain_expect.py --, field for field, at the smallest shapes where each piece can go wrong."""
import ctypes as C
import functools

import numpy as np
import pytest

import align_expect as AE
import fm_expect as F
import fm_path_graphs as P
import gbwt_rs_amd as G
import sa_expect as A
import seed_expect as E
from gbwt_rs_amd import _lib
from test_chains_cpu import SETTINGS, case_reads, replaced
from test_gpu_seeds import GUARD, guarded, view

pytestmark = pytest.mark.gpu

MOST = 1 << 20
GRAPH = P.tangle_small()
ORDERS = P.orders(GRAPH)


@functools.lru_cache(maxsize=None)
def brute(text):
    sa = F.suffix_array(text)
    sa.setflags(write=False)
    return sa


def alignment_tuples(alignments):
    assert alignments.dtype == G.ALIGNMENT_DTYPE
    return list(zip(*(alignments[name].tolist() for name in G.ALIGNMENT_DTYPE.names)))


def check(fm, text, reads, bounds=None, sa=None, **options):
    """One request against the yardstick: every output field, and the counts of the info."""
    want = AE.expected_rows(text, brute(text) if sa is None else sa, reads, bounds=bounds, **options)
    read_offsets, alignments, cigar_offsets, cigars = fm.alignments(reads, **options)
    assert read_offsets.dtype == cigar_offsets.dtype == np.uint64 and cigars.dtype == np.uint32
    assert read_offsets.tolist() == want["read_offsets"], options
    assert alignment_tuples(alignments) == want["alignments"], options
    assert cigar_offsets.tolist() == want["cigar_offsets"], options
    assert cigars.tolist() == want["cigars"], options
    info = fm.last_align_info()
    total = len(want["alignments"])
    assert (info["items"], info["chains"], info["alignments"], info["wide"], info["unreachable"], info["cells"], info["cigar_ops"]) == \
        (want["items"], total, total, want["wide"], want["unreachable"], want["cells"], len(want["cigars"])), options
    assert info["lds_alignments"] + info["global_alignments"] == total - want["wide"]
    assert info["planned_scratch_bytes"] == info["peak_scratch_bytes"] > 0
    assert info["text_bytes"] == max(len(text), 256) and info["trace_ms"] == 0
    return want, info


def cigar_of(want, a):
    return AE.cigar_string(want["cigars"][want["cigar_offsets"][a]:want["cigar_offsets"][a + 1]])


# ---- 1: the first case ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", [8, 16])
def test_the_first_case(band):
    text = A.mutated_rows(4, 300, 3)
    reads = case_reads(text)
    fm = G.FMIndex.from_text(text, keep_text=True)
    for max_gap, max_skew, gap_cost, min_score in SETTINGS:
        want, info = check(fm, text, reads, min_length=5, strands=G.STRAND_BOTH, max_occurrences=MOST, max_gap=max_gap, max_skew=max_skew, gap_cost=gap_cost, min_score=min_score,
                           band=band)
        assert info["dp_ms"] > 0 and info["rows_ms"] > 0 and info["select_ms"] > 0
        if (max_gap, max_skew, gap_cost, min_score, band) == (1000, 50, 1, 1, 8):
            firsts = [want["read_offsets"][k] for k in range(4)]
            assert [(want["alignments"][a][3], cigar_of(want, a)) for a in firsts] == [(0, "150="), (2, "40=1X49=1X59="), (3, "69=3D78="), (5, "64=2I2=1I3=1I1=1I80=")]
            assert [want["alignments"][a][:2] for a in firsts] == [(10, 160), (20, 170), (30, 180), (30, 180)]
            assert want["unreachable"] > 0 and {row[6] for row in want["alignments"]} == {1, 2}
        assert want["read_offsets"][6:] == [want["read_offsets"][6]] * 4          # the empty read, A and ZZZ: no chains, empty rows
    fm.close()


# ---- 2: chunk edges of the band -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [63, 64, 65, 128, 129])
def test_chunk_edges_of_the_band(width):
    text = A.mutated_rows(1, 600, 0, seed=11)
    plain = replaced(text[100:250], (40, 90))                                     # one diagonal: spread 0
    long = text[300:450]
    shifted = replaced(long[:70] + long[71:], (20, 120))                          # a base deleted: two diagonals, spread 1
    options = dict(min_length=10, strands=G.STRAND_FORWARD, max_occurrences=MOST, max_gap=1000, max_skew=50, max_alignments=1)
    fm = G.FMIndex.from_text(text, keep_text=True)
    for read in (plain, shifted):
        chains = AE.X.expected_rows(text, brute(text), [read], 10, E.FORWARD, MOST, 1000, 50, 1, 1)
        members = chains["matches"][chains["match_offsets"][0]:chains["match_offsets"][1]]
        spread = max(y - x for y, x, _ in members) - min(y - x for y, x, _ in members)
        assert spread == (0 if read is plain else 1)
        if (width - 1 - spread) % 2:
            continue
        band = (width - 1 - spread) // 2
        want, _ = check(fm, text, [read], band=band, max_width=width, **options)
        assert want["alignments"][0][4:6] == (width, AE.OK) and want["alignments"][0][3] == (2 if read is plain else 3)
        narrow, info = check(fm, text, [read], band=band, max_width=width - 1, **options)
        assert narrow["alignments"][0][3:6] == (AE.INF, width, AE.WIDE) and narrow["cigars"] == [] and info["wide"] == 1 and info["cells"] == 0
    fm.close()


# ---- 3: both sides of the tile --------------------------------------------------------------------------------------------------------------

def test_both_sides_of_the_tile():
    probe = G.FMIndex.from_text(b"ACGT")
    tile = probe.last_align_info()["tile_bytes"]
    assert probe.last_align_info()["text_bytes"] == 0
    probe.close()
    assert tile % 8 == 0 and 1024 <= tile <= 65536
    rows = tile // 8                                                              # W = 17: two words a row
    text = A.mutated_rows(1, rows + 1000, 0, seed=17)
    options = dict(min_length=24, strands=G.STRAND_FORWARD, max_occurrences=MOST, max_gap=2000, max_skew=50, max_alignments=1, band=8)
    fm = G.FMIndex.from_text(text, keep_text=True)
    splits = []
    for length in (rows, rows + 1):
        read = replaced(text[100:100 + length], (50, length // 2, length - 60))
        want, info = check(fm, text, [read], **options)
        assert want["alignments"][0][3:6] == (3, 17, AE.OK) and length * 2 * 4 == tile + 8 * (length - rows)
        splits.append((info["lds_alignments"], info["global_alignments"]))
    assert splits == [(1, 0), (0, 1)]
    # beyond the tile with an indel, next to one inside it: both ways in one request
    long = text[150:150 + rows + 100]
    want, info = check(fm, text, [long[:400] + long[403:], text[20:170]], **options)
    assert [row[3] for row in want["alignments"]] == [3, 0] and "3D" in cigar_of(want, 0) and (info["lds_alignments"], info["global_alignments"]) == (1, 1)
    # a text window that no LDS stages: rows + 700 text bytes under the band
    want, info = check(fm, text, [replaced(text[200:200 + rows + 700], (800,))], **options)
    assert want["alignments"][0][3:6] == (1, 17, AE.OK) and info["global_alignments"] == 1
    fm.close()


# ---- 4: path level --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev():
    handle = G.GBZ.from_gfa_text(GRAPH.gfa())
    assert handle.paths() == GRAPH.paths()
    yield handle
    handle.close()


@functools.lru_cache(maxsize=None)
def path_case(name, endmarker):
    order = ORDERS[name]
    text, bounds = GRAPH.text(order, endmarker), GRAPH.bounds(order)
    label = GRAPH.labels[P.LONG_NODE]
    edited = label[:90] + label[92:150]
    reads = P.reads_across(GRAPH, order, endmarker) + [label, P.reverse_complement(label), replaced(edited, (30, 100))]
    if name == "single":
        base = GRAPH.row_text(P.ONE_STEP_PATH)
        reads = [base, base + base, P.reverse_complement(base), b"", b"ZZZ"]
    return order, text, bounds, brute(text), reads


@pytest.mark.parametrize("endmarker", P.ENDMARKERS)
@pytest.mark.parametrize("name", ["all", "duplicate", "single"])
def test_path_level(dev, name, endmarker):
    order, text, bounds, sa, reads = path_case(name, endmarker)
    offsets, data = dev.path_sequences(order, endmarker=endmarker)
    assert offsets.tolist() == bounds and bytes(data) == text                     # the fixture itself
    fm = dev.fm_index(order, endmarker=endmarker)
    with pytest.raises(G.GbwtHipError) as e:
        fm.alignments(reads, max_occurrences=MOST)
    assert e.value.status == _lib.UNSUPPORTED and "gbwt_hip_fm_keep_path_text" in str(e.value) and "gbwt_hip_fm_set_text" in str(e.value)
    dev.path_sequences(order[:1], endmarker=7)                                    # another request for bases on the workspace in between
    fm.keep_text()
    options = dict(min_length=1 if name == "single" else 4, strands=G.STRAND_BOTH, max_occurrences=MOST, max_gap=1000, max_skew=50)
    seen_none = seen_insertions = False
    for band in (16, 24):
        want, info = check(fm, text, reads, bounds=bounds, sa=sa, band=band, **options)
        assert info["text_bytes"] == max(len(text), 256) and fm.info()["index_bytes"] == fm.info()["planned_index_bytes"]
        assert want["alignments"] or name == "single"
        for a, row in enumerate(want["alignments"]):
            lo, hi = bounds[row[7]], bounds[row[7] + 1] - 1
            if row[5] == AE.OK:                                                   # no alignment holds an endmarker position
                assert lo <= row[0] <= row[1] <= hi, (name, endmarker, row)
                seen_insertions |= row[1] == hi and cigar_of(want, a).endswith("I")
            seen_none |= row[5] == AE.NONE
        if name == "duplicate":                                                   # the two copies of an id: the same alignments but for `path` and the offset of the copy
            first, copy = 0, len(order) - 1
            assert order[first] == order[copy]
            gaps = len(reads[:-3]) // 4                                          # reads_across: per path end one read without a byte in between, then those with one
            plain = [k for k in range(len(reads)) if k >= len(reads) - 3 or k % gaps == 0]      # (a seed through an endmarker depends on what follows the copy)
            read_of = lambda a: int(np.searchsorted(want["read_offsets"], a, side="right")) - 1
            relative = lambda place: sorted((row[0] - bounds[place] if row[5] == AE.OK else 0, row[1] - bounds[place] if row[5] == AE.OK else 0, row[3], row[4], row[5], row[6],
                                             cigar_of(want, a)) for a, row in enumerate(want["alignments"]) if row[7] == place and read_of(a) in plain)
            assert relative(first) == relative(copy) != []
    if name == "single":
        assert bounds == [0, 2] and len(text) == 2
        want, _ = check(fm, text, reads, bounds=bounds, sa=sa, band=0, **options)
        assert [row[:2] + row[3:6] for row in want["alignments"][:1]] == [(0, 1, 0, 1, AE.OK)] and cigar_of(want, 0) == "1="
    else:
        assert seen_none and seen_insertions                                      # reads across a path's end: beyond the band, and inside it
    fm.close()


# ---- 5: max_alignments ----------------------------------------------------------------------------------------------------------------------

def test_max_alignments_and_empty_rows():
    text = A.mutated_rows(4, 300, 3)
    reads = case_reads(text)
    fm = G.FMIndex.from_text(text, keep_text=True)
    options = dict(min_length=5, strands=G.STRAND_BOTH, max_occurrences=MOST, max_gap=1000, max_skew=50, band=8)
    sizes = {}
    for most in (0, 1, 2):
        want, _ = check(fm, text, reads, max_alignments=most, **options)
        sizes[most] = [want["read_offsets"][k + 1] - want["read_offsets"][k] for k in range(len(reads))]
        assert sizes[most][6:] == [0, 0, 0]
    assert max(sizes[1]) == 2 and max(sizes[2]) == 4 and max(sizes[0]) > 4 and sizes[1][0] == 2     # one per strand
    assert [a.tolist() for a in fm.alignments([], max_occurrences=5)] == [[0], [], [0], []]
    assert [a.tolist() for a in fm.alignments([b"", b"ZZZ"], max_occurrences=5)] == [[0, 0, 0], [], [0], []]
    fm.close()


# ---- 6: the protocol ------------------------------------------------------------------------------------------------------------------------

def test_size_query_fill_protocol_and_requests():
    text = A.mutated_rows(4, 300, 3)
    reads = case_reads(text)
    offsets, data = G.api._patterns_csr(reads)
    want = AE.expected_rows(text, brute(text), reads, 5, E.BOTH, MOST, 1000, 50, 1, 1, band=8, max_alignments=2)
    n_a, n_c = len(want["alignments"]), len(want["cigars"])
    fm = G.FMIndex.from_text(text, keep_text=True)
    assert fm.last_align_info()["requests"] == 0
    L, total_rows, total_cigars = fm._L, C.c_uint64(0), C.c_uint64(0)
    seed_opts, chain_opts, align_opts = _lib.FmSeedOptions(5, 3, MOST, 0, 0), _lib.FmChainOptions(1000, 50, 1, 1, 0, 0, 0), _lib.FmAlignOptions(8, 0, 2, 0, 0)
    read_offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    args = (fm._fm, offsets.ctypes.data, data.ctypes.data, len(reads), C.byref(seed_opts), C.byref(chain_opts), C.byref(align_opts), read_offsets.ctypes.data)
    _lib.check(L.gbwt_hip_fm_alignments(*args, None, 0, C.byref(total_rows), None, None, 0, C.byref(total_cigars)))        # the size query computes
    sized = fm.last_align_info()
    assert (total_rows.value, total_cigars.value) == (n_a, n_c) and sized["requests"] == 1 and sized["alignments"] == n_a and read_offsets.tolist() == want["read_offsets"]
    assert sized["chains_ms"] > 0 and sized["dp_ms"] > 0 and fm.last_chain_info()["requests"] == 1 and fm.last_seed_info()["requests"] == 1
    rows, cigar_offsets, cigars = np.zeros(n_a, dtype=G.ALIGNMENT_DTYPE), np.zeros(n_a + 1, dtype=np.uint64), np.zeros(n_c, dtype=np.uint32)
    # a capacity that is too small: the totals, and nothing written
    read_offsets[:] = 77
    for capacity, cigar_capacity, word in ((n_a - 1, n_c, b"alignment capacity"), (n_a, n_c - 1, b"cigar capacity")):
        a, b = C.c_uint64(0), C.c_uint64(0)
        status = L.gbwt_hip_fm_alignments(*args, rows.ctypes.data, capacity, C.byref(a), cigar_offsets.ctypes.data, cigars.ctypes.data, cigar_capacity, C.byref(b))
        assert status == _lib.CAPACITY and (a.value, b.value) == (n_a, n_c) and word in L.gbwt_hip_last_error()
        assert not rows.view(np.uint8).any() and not cigar_offsets.any() and not cigars.any() and (read_offsets == 77).all()
    _lib.check(L.gbwt_hip_fm_alignments(*args, rows.ctypes.data, n_a, C.byref(total_rows), cigar_offsets.ctypes.data, cigars.ctypes.data, n_c, C.byref(total_cigars)))   # the fill only copies
    assert fm.last_align_info() == sized
    assert alignment_tuples(rows) == want["alignments"] and cigar_offsets.tolist() == want["cigar_offsets"] and cigars.tolist() == want["cigars"]
    # chains and seeds with the same arguments compute nothing: their rows are those of the alignments request
    chains = fm.chains(reads, min_length=5, strands=G.STRAND_BOTH, max_occurrences=MOST, max_gap=1000, max_skew=50)
    assert fm.last_chain_info()["requests"] == 1 and chains[1].size == len(want["chain_rows"]["chains"])
    assert [tuple(int(v) for v in row) for row in chains[1].tolist()] == want["chain_rows"]["chains"]
    fm.seeds(reads, min_length=5, strands=G.STRAND_BOTH, max_occurrences=MOST)
    assert fm.last_seed_info()["requests"] == 1
    # other align options are another request, on the same chains
    check(fm, text, reads, min_length=5, strands=G.STRAND_BOTH, max_occurrences=MOST, max_gap=1000, max_skew=50, band=16)
    again = fm.last_align_info()
    assert again["requests"] == 2 and again["chains_ms"] == 0 and fm.last_chain_info()["requests"] == 1
    fm.alignments(reads, min_length=5, strands=G.STRAND_BOTH, max_occurrences=MOST, max_gap=1000, max_skew=50, band=16)
    assert fm.last_align_info() == again
    # the device form: the rows of the host form in HBM, the caller's buffers as they were
    import torch
    options = dict(min_length=5, max_occurrences=MOST, max_gap=100, max_skew=10, gap_cost=2, min_score=20, band=8)
    host = fm.alignments(reads, **options)
    t_off, p_off = guarded(offsets, 8)
    t_dat, p_dat = guarded(data, 3)
    torch.cuda.synchronize()
    out = fm.alignments_device(p_off, p_dat, len(reads), data.size, **options)
    assert out.m == len(reads) and out.total_alignments == host[1].size > 0 and out.total_cigars == host[3].size > 0
    assert np.array_equal(view(out.d_read_offsets, len(reads) + 1), host[0]) and np.array_equal(view(out.d_cigar_offsets, out.total_alignments + 1), host[2])
    assert np.array_equal(view(out.d_alignments, 5 * out.total_alignments).view(G.ALIGNMENT_DTYPE), host[1])
    assert np.array_equal(view(out.d_cigars, out.total_cigars // 2).view(np.uint32), host[3][:2 * (out.total_cigars // 2)])   # (whole u64 words: nothing behind the row is read)
    for t, lead, payload in ((t_off, 8, 8 * (len(reads) + 1)), (t_dat, 3, data.size)):
        raw = t.cpu().numpy()
        assert (raw[:lead] == GUARD).all() and (raw[lead + payload:] == GUARD).all() and raw.size == lead + payload + 16
    assert np.array_equal(t_off.cpu().numpy()[8:-16].view(np.uint64), offsets) and np.array_equal(t_dat.cpu().numpy()[3:-16], data)
    fm.close()


# ---- 7: the text ----------------------------------------------------------------------------------------------------------------------------

def test_the_text():
    text = A.mutated_rows(4, 300, 3)
    reads = case_reads(text)[:4]
    options = dict(min_length=5, strands=G.STRAND_FORWARD, max_occurrences=MOST, max_gap=1000, max_skew=50, band=8, max_alignments=1)
    fm = G.FMIndex.from_text(text)
    before = fm.info()
    assert fm.last_align_info()["text_bytes"] == 0
    with pytest.raises(G.GbwtHipError) as e:
        fm.alignments(reads, **options)
    assert e.value.status == _lib.UNSUPPORTED and "gbwt_hip_fm_set_text" in str(e.value) and fm.last_align_info()["requests"] == 0
    for wrong in (text[:-1], text + b"A"):
        with pytest.raises(G.GbwtHipError) as e:
            fm.set_text(wrong)
        assert e.value.status == _lib.BAD_ARGUMENT
    changed = bytearray(text)
    changed[500] = ord("A") if changed[500] != ord("A") else ord("C")
    with pytest.raises(G.GbwtHipError) as e:
        fm.set_text(bytes(changed))
    assert e.value.status == _lib.INVALID_DATA and fm.last_align_info()["text_bytes"] == 0
    # a text with the histogram of the index passes the check and is what the alignments read: a second call replaces it
    swapped = bytearray(text)
    at = next(k for k in range(40, 60) if text[k] != text[k + 1])
    swapped[at], swapped[at + 1] = swapped[at + 1], swapped[at]
    fm.set_text(bytes(swapped))
    first = fm.alignments(reads, **options)
    assert first[1]["edit_distance"].tolist()[0] == 2 and AE.cigar_string(first[3][int(first[2][0]):int(first[2][1])]) == f"{at - 10}=2X{158 - at}="
    fm.set_text(text)
    want, info = check(fm, text, reads, **options)
    assert [row[3] for row in want["alignments"]] == [0, 2, 3, 5]
    after = fm.info()
    assert after["index_bytes"] == after["planned_index_bytes"] == before["index_bytes"] and info["text_bytes"] == len(text)
    fm.close()
    kept = G.FMIndex.from_text(text, keep_text=True)
    check(kept, text, reads, **options)
    kept.close()
    lean = G.FMIndex.from_text(text, count_only=True, keep_text=True)
    with pytest.raises(G.GbwtHipError) as e:
        lean.alignments(reads, **options)
    assert e.value.status == _lib.UNSUPPORTED
    lean.close()
