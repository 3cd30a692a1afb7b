"""The FM-index family of paths -- GBZ.suffix_array, GBZ.fm_index (count, locate_csr, graph_positions_csr), seeds(graph=True) and chains -- on
graphs built for its edge cases (tests/fm_path_graphs.py): path lists that are subsets, reversed or name an id twice, a one-node path of two
text bytes, endmarkers that are no 0 and one that is also a base, nodes read in reverse and twice in a row, labels around the seed stride and
one longer than a read, node ids at the top of the range, items of exactly the DP tile and two more whose windows jump over a path, and other
requests between two requests on the owner's workspace.  The handles come from GBZ.from_gfa_text; every test first holds
dev.path_sequences against the helper's text, and every expectation is computed from the helper's own labels and walks with the
yardsticks fm_expect, seed_expect, chain_expect and sa_expect -- none from dev.tag_array or dev.path_sequences.  What the cases must
contain for a pass to mean something is pinned in tests/test_fm_path_graphs_cpu.py and asserted here again from the yardstick."""
import ctypes as C
import functools

import numpy as np
import pytest

import chain_expect as X
import fm_expect as F
import fm_path_graphs as P
import gbwt_rs_amd as G
import sa_expect as A
import seed_expect as E
import shifted_graphs as SG
from gbwt_rs_amd import _lib
from test_gpu_chains import check as check_chains
from test_gpu_seeds import as_tuples, check_hits, check_seeds, rows_of, stride

pytestmark = pytest.mark.gpu

MOST = 1 << 20
GRAPH = P.tangle_small()
ORDERS = P.orders(GRAPH)
LONG_FORWARD, LONG_REVERSE = P.LONG_NODE << 11, (P.LONG_NODE << 11) | (1 << 10)
CHAINS = dict(min_length=4, strands=G.STRAND_BOTH, max_occurrences=MOST, max_gap=1000, max_skew=50)
PERIODIC = dict(min_length=5, strands=G.STRAND_FORWARD, max_occurrences=MOST, max_gap=400, max_skew=8)


@functools.lru_cache(maxsize=None)
def case_of(name, endmarker):
    """The yardstick of one (path list, endmarker): computed once, shared by the tests, never written to."""
    return P.Case(GRAPH, ORDERS[name], endmarker)


def check_text(dev, graph, order, endmarker):
    """The fixture itself: the bases the device reads for these paths are the helper's text."""
    offsets, data = dev.path_sequences(order, endmarker=endmarker)
    assert offsets.tolist() == graph.bounds(order) and bytes(data) == graph.text(order, endmarker), (order, endmarker)


@pytest.fixture(scope="module")
def dev():
    assert stride() == P.STRIDE                                                  # the reads are cut around the library's K
    handle = G.GBZ.from_gfa_text(GRAPH.gfa())
    assert handle.paths() == GRAPH.paths()
    yield handle
    handle.close()


@pytest.fixture(scope="module", params=[(name, e) for name in P.ORDER_NAMES for e in P.ENDMARKERS], ids=lambda p: f"{p[0]}-{p[1]}")
def indexed(request, dev):
    """(name, case, dev, the index of the case's paths); the index is closed before the handle."""
    name, endmarker = request.param
    c = case_of(name, endmarker)
    check_text(dev, GRAPH, c.order, endmarker)
    fm = dev.fm_index(c.order, endmarker=endmarker)
    yield name, c, dev, fm
    fm.close()


# ---- C1: orders and endmarkers ------------------------------------------------------------------------------------------------------------------

def test_suffix_array_bwt_and_runs(indexed):
    name, c, dev, fm = indexed
    check_text(dev, GRAPH, c.order, c.endmarker)
    sa, bwt, runs = dev.suffix_array(c.order, endmarker=c.endmarker, return_bwt=True)
    assert np.array_equal(sa, c.sa), name
    want = A.bwt(c.text, c.sa, c.endmarker)
    assert np.array_equal(bwt, want) and runs == A.runs(want), name
    info = fm.info()
    assert info["n"] == len(c.text) and info["path_level"] == 1 and info["suffix_array_ms"] == 0
    assert info["primary"] == int(np.flatnonzero(c.sa == 0)[0])


def check_positions(fm, c, patterns, sa_tags, what):
    """count, locate_csr and graph_positions_csr of these patterns against the brute-force suffix array and the tags of its rows."""
    want_ranges, want_rows = F.expected(c.text, c.sa, patterns)
    assert np.array_equal(fm.count(patterns).astype(np.int64), want_ranges), what
    offsets, positions = fm.locate_csr(patterns)
    assert offsets[0] == 0 and np.array_equal(np.diff(offsets.astype(np.int64)), want_ranges[:, 1] - want_ranges[:, 0]), what
    for p, got, want in zip(patterns, rows_of(offsets, positions), want_rows):
        assert np.array_equal(got, want), (what, p)
    t_offsets, tags = fm.graph_positions_csr(patterns, unique=False)
    u_offsets, u_tags = fm.graph_positions_csr(patterns, unique=True)
    assert np.array_equal(t_offsets, offsets), what
    for k, (p, (lo, hi)) in enumerate(zip(patterns, want_ranges)):
        assert np.array_equal(tags[int(t_offsets[k]):int(t_offsets[k + 1])], sa_tags[lo:hi]), (what, p)
        assert np.array_equal(u_tags[int(u_offsets[k]):int(u_offsets[k + 1])], np.unique(sa_tags[lo:hi])), (what, p)
    return want_ranges


def test_counts_positions_and_graph_positions(indexed):
    name, c, dev, fm = indexed
    check_text(dev, GRAPH, c.order, c.endmarker)
    patterns = F.text_patterns(c.text)
    assert patterns[0] == b"" and len(patterns) % 64 != 0
    check_positions(fm, c, patterns, c.sa_tags, name)                             # (the empty pattern: every tag of the text, in SA order)
    # by hand: the first base of the 200-base node read in reverse, and its last base read forward
    for orientation, offset, tag in ((1, 0, LONG_REVERSE), (0, P.LONG_LENGTH - 1, LONG_FORWARD + P.LONG_LENGTH - 1)):
        visits = GRAPH.visits(c.order, P.LONG_NODE, orientation)
        assert visits or name == "single"
        for k, step in visits:
            at = c.bounds[k] + GRAPH.step_starts(c.order[k])[step] + offset
            assert tag in fm.graph_positions(c.text[at:at + 14]).tolist(), (name, k, step)
    assert (LONG_REVERSE in fm.graph_positions(P.reverse_complement(GRAPH.labels[P.LONG_NODE])).tolist()) == (name != "single")
    # an endmarker is 0, once per path of the list -- also where the endmarker byte is a base
    marks = fm.graph_positions(bytes([c.endmarker]), unique=False)
    assert int(np.count_nonzero(marks == 0)) == len(c.order) and fm.graph_positions(bytes([c.endmarker]))[0] == 0
    if c.endmarker != 65:
        assert marks.tolist() == [0] * len(c.order) and fm.graph_positions(bytes([c.endmarker])).tolist() == [0]
    else:
        assert marks.size == c.text.count(b"A") >= len(c.order)


def test_seeds_and_their_graph_positions(indexed):
    name, c, dev, fm = indexed
    check_text(dev, GRAPH, c.order, c.endmarker)
    assert len(c.reads) <= 200 and c.reads_without_seeds(), name
    assert c.seeds_in_two_segments() or name == "single"
    for min_length in (1, 5):
        check_seeds(fm, c.text, c.reads, min_length, G.STRAND_BOTH, name)
    want = [s[1:] for s in c.seeds()]
    check_hits(fm, c.sa, c.reads, MOST)
    for most in (MOST, 2):
        seeds, over = check_hits(fm, c.sa, c.reads, most, values=c.sa_tags, graph=True)
        assert as_tuples(seeds) == want, name
        assert over == sum(1 for s in want if s[4] - s[3] > most) and (over > 0) == (most == 2 and name != "single")
    if name != "single":
        across = c.seeds_over_a_path_end()                                        # the read with the endmarker byte in it occurs across a path's end
        assert across and (c.endmarker != 65 or any(0 not in c.reads[s[0]] and 36 not in c.reads[s[0]] for s, _ in across))


def test_chains_stay_inside_their_paths(indexed):
    name, c, dev, fm = indexed
    check_text(dev, GRAPH, c.order, c.endmarker)
    want, info = check_chains(fm, c.text, c.reads, bounds=c.bounds, **CHAINS)
    assert info["path_offset_bytes"] == max(8 * len(c.bounds), 256)
    if name == "single":
        assert want["chains"] == [] and len(c.text) == 2
        return
    assert any(row[5] >= 2 for row in want["chains"]) and len({row[7] for row in want["chains"]}) > 1, name
    bounds = c.bounds
    if name == "reversed":                                                        # the whole text of two paths as a read: an item above the tile, over global memory, with segments
        assert max(len(X.matches_of(c.text, c.sa, read, strand, 4)) for read in c.reads[-20:] for strand in (E.FORWARD, E.REVERSE)) > tile()
    for row, first, last in zip(want["chains"], want["match_offsets"][:-1], want["match_offsets"][1:]):     # the rows the device gave: check() held them equal
        assert all(bounds[row[7]] <= y < bounds[row[7] + 1] for y, _, _ in want["matches"][first:last]), (name, row)
    if c.endmarker == 65:                                                         # seeds run through a path's end, chains do not join over it
        assert any(c.reads[s[0]].count(b"A") and p + s[2] - s[1] > bounds[c.segment_of(p) + 1] for s, p in c.seeds_over_a_path_end())
    if name == "duplicate":                                                       # segments 7 and 8 hold path 7: the same chains, once per copy
        assert c.order[7] == c.order[8]
        distance = bounds[8] - bounds[7]
        by_read = [(k,) + row for k in range(len(c.reads)) for row in want["chains"][want["read_offsets"][k]:want["read_offsets"][k + 1]]]
        first, second = sorted(r for r in by_read if r[8] == 7), sorted(r for r in by_read if r[8] == 8)
        assert first and [(r[0], r[1] + distance, r[2] + distance) + r[3:8] + (8,) for r in first] == second


# ---- C2: node ids moved up ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", SG.SHIFT_NAMES)
def test_node_ids_moved_up(shift):
    c = case_of("all", 0)
    d = SG.SHIFTS(P.LONG_NODE)[shift]
    dev = G.GBZ.from_gfa_text(SG.shift_gfa(GRAPH.gfa(), d))
    check_text(dev, GRAPH, c.order, 0)                                            # the bases do not move
    moved = SG.move_tags(c.sa_tags, d)
    assert int(np.count_nonzero(moved == 0)) == len(c.order)
    if shift == "top":
        assert int(moved.max()) > 1 << 41 and int(moved.max()) >> 11 == SG.MAX_NODE_ID
    sa, bwt, runs = dev.suffix_array(c.order, endmarker=0, return_bwt=True)
    assert np.array_equal(sa, c.sa) and np.array_equal(bwt, A.bwt(c.text, c.sa, 0)) and runs == A.runs(bwt)
    fm = dev.fm_index(c.order)
    check_positions(fm, c, F.text_patterns(c.text), moved, shift)
    every = fm.graph_positions(b"", unique=False)
    assert np.array_equal(every, moved) and (shift != "top" or int(every.max()) > 1 << 41)
    assert ((P.LONG_NODE + d) << 11) | (1 << 10) in fm.graph_positions(P.reverse_complement(GRAPH.labels[P.LONG_NODE])).tolist()
    check_seeds(fm, c.text, c.reads, 1, G.STRAND_BOTH, shift)
    for most in (MOST, 2):
        seeds, _ = check_hits(fm, c.sa, c.reads, most, values=moved, graph=True)
        assert as_tuples(seeds) == [s[1:] for s in c.seeds()], shift
    check_chains(fm, c.text, c.reads, bounds=c.bounds, **CHAINS)
    fm.close()
    dev.close()


# ---- C3: segments meet wide windows and the tile ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tile():
    probe = G.FMIndex.from_text(b"ACGT")
    matches = probe.last_chain_info()["tile_matches"]
    probe.close()
    assert 376 <= matches <= 2000                                                 # the lists below hold a first path of 120 repeats, and a text below 3 000 bytes
    return matches


@pytest.mark.parametrize("which,endmarker", [("tile", 0), ("tile + 2", 0), ("two paths", 0), ("tile + 2", 36)])
def test_segments_meet_wide_windows_and_the_tile(which, endmarker):
    count = {"tile": tile(), "tile + 2": tile() + 2, "two paths": 132}[which]
    reps = [40, 30] if which == "two paths" else P.periodic_reps_for(count)
    graph, order = P.periodic(reps), list(range(len(reps)))
    text, bounds = graph.text(order, endmarker), graph.bounds(order)
    assert len(text) <= 3000 and (which == "two paths" or (3 in reps and 2 in reps))
    dev = G.GBZ.from_gfa_text(graph.gfa())
    check_text(dev, graph, order, endmarker)
    read = P.PERIODIC_READ
    # from the yardstick: the item has exactly this many matches, its windows are wider than two waves (one and a part for the two paths),
    # and the first match behind a path leaves more than that many below its window at once
    matches = X.matches_of(text, F.suffix_array(text), read, E.FORWARD, 5)
    sizes, jumps = P.window_sizes(matches, bounds, 400), np.diff(P.window_starts(matches, bounds, 400))
    wide = 64 if which == "two paths" else 128
    assert len(matches) == count == P.periodic_matches(reps) and sizes.max() > wide and jumps.max() > wide
    assert (count > tile()) == (which == "tile + 2")                              # at the tile: staged; two more: over global memory
    fm = dev.fm_index(order, endmarker=endmarker)
    want, info = check_chains(fm, text, [read], bounds=bounds, **PERIODIC)
    assert info["matches"] == count and info["tile_matches"] == tile() and info["items"] == 1
    assert all(bounds[row[7]] <= row[0] and row[1] <= bounds[row[7] + 1] - 1 for row in want["chains"])       # no chain crosses a bound
    assert sorted({row[7] for row in want["chains"]}) == [k for k, r in enumerate(reps) if r >= 3]
    # one below the item's count: no chains, and the item is counted
    skipped, _ = check_chains(fm, text, [read], bounds=bounds, max_matches=count - 1, **PERIODIC)
    assert skipped["skipped_items"] == 1 and skipped["chains"] == [] and skipped["read_offsets"] == [0, 0]
    kept, _ = check_chains(fm, text, [read], bounds=bounds, max_matches=count, **PERIODIC)
    assert kept["chains"] == want["chains"]
    fm.close()
    # the segments matter: the same bytes as a plain text join over the bounds
    plain = G.FMIndex.from_text(text, sentinel=endmarker)
    joined, plain_info = check_chains(plain, text, [read], **PERIODIC)
    assert plain_info["matches"] == count and plain_info["pairs"] > info["pairs"] and joined["chains"] != want["chains"] and len(joined["chains"]) != len(want["chains"])
    assert any(any(row[0] < b <= row[1] - 1 for b in bounds[1:-1]) for row in joined["chains"])
    plain.close()
    dev.close()


# ---- C5: the owner's workspace ----------------------------------------------------------------------------------------------------------------------

OTHER_IDS = [3, 5, 2, 7]


def workspace_case():
    c = case_of("subset", 0)
    patterns = [p for p in F.text_patterns(c.text) if len(p) >= 3][:90] + [b"A", b""]
    want_ranges, _ = F.expected(c.text, c.sa, patterns)
    flat = np.concatenate([c.sa_tags[lo:hi] for lo, hi in want_ranges])
    unique = np.concatenate([np.unique(c.sa_tags[lo:hi]) for lo, hi in want_ranges])
    assert set(OTHER_IDS) - set(c.order) and flat.size > unique.size
    return c, patterns, flat, unique


def test_other_requests_between_two_on_the_owners_workspace(dev):
    c, patterns, flat, unique = workspace_case()
    check_text(dev, GRAPH, c.order, 0)
    reads = c.reads
    fm = dev.fm_index(c.order)
    before = fm.graph_positions_csr(patterns)
    before_unique = fm.graph_positions_csr(patterns, unique=True)
    assert np.array_equal(before[1], flat) and np.array_equal(before_unique[1], unique)
    seeds_before = fm.seeds(reads, max_occurrences=50, graph=True)
    queries, requests = fm.info()["queries"], fm.last_seed_info()["requests"]
    # tags, bases and a suffix array of other paths on the workspace the index asks for its tags
    other_text, other_tags = GRAPH.text(OTHER_IDS, 36), GRAPH.tags(OTHER_IDS)
    every = np.arange(other_tags.size, dtype=np.uint64)
    assert np.array_equal(dev.tag_array(OTHER_IDS, every), other_tags)
    offsets, data = dev.path_sequences(OTHER_IDS, G.REVERSE, 255)
    rows = [P.reverse_complement(GRAPH.row_text(p)) + b"\xff" for p in OTHER_IDS]
    assert bytes(data) == b"".join(rows) and offsets.tolist() == np.cumsum([0] + [len(r) for r in rows]).tolist()
    assert np.array_equal(dev.suffix_array(OTHER_IDS, endmarker=36), F.suffix_array(other_text))
    sa_info = dev.last_suffix_array_info()
    assert sa_info["n"] == len(other_text) != len(c.text)
    # the index answers as before, and computes: the rows it held were those of the unique request
    after = fm.graph_positions_csr(patterns)
    assert fm.info()["queries"] == queries + 1
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], flat)
    after_unique = fm.graph_positions_csr(patterns, unique=True)
    assert np.array_equal(after_unique[0], before_unique[0]) and np.array_equal(after_unique[1], unique)
    check_hits(fm, c.sa, reads, 2, values=c.sa_tags, graph=True)                  # (another request first: the one from before is computed again)
    seeds, _ = check_hits(fm, c.sa, reads, 50, values=c.sa_tags, graph=True)
    assert as_tuples(seeds) == [s[1:] for s in c.seeds()] and fm.last_seed_info()["requests"] == requests + 2
    seeds_after = fm.seeds(reads, max_occurrences=50, graph=True)
    assert all(np.array_equal(a, b) for a, b in zip(seeds_before, seeds_after))
    assert np.array_equal(dev.tag_array(OTHER_IDS, every[::-1]), other_tags[::-1])                      # ... between two requests of the index again
    check_chains(fm, c.text, reads, bounds=c.bounds, **CHAINS)
    check_hits(fm, c.sa, reads, 2, values=c.sa_tags, graph=True)
    assert np.array_equal(fm.graph_positions_csr(patterns)[1], flat)
    # the requests in between are still right, and the suffix array on the workspace is still that of the other paths
    assert np.array_equal(dev.tag_array(OTHER_IDS, every), other_tags)
    assert dev.last_suffix_array_info() == sa_info
    fm.close()


def test_a_second_workspace_of_the_same_handle(dev):
    c, patterns, flat, unique = workspace_case()
    check_text(dev, GRAPH, c.order, 0)
    L = dev._L
    fm = dev.fm_index(c.order)
    first = fm.graph_positions_csr(patterns)
    assert np.array_equal(first[1], flat)
    second = C.c_void_p()
    _lib.check(L.gbwt_hip_workspace_create(dev._h, C.byref(second)))
    try:
        offsets, data = G.api._patterns_csr(patterns)
        queries = fm.info()["queries"]
        got_unique = fm._rows(lambda o, b, m, *rest: L.gbwt_hip_fm_graph_positions(fm._fm, dev._h, second, o, b, m, 1, *rest), offsets, data)
        got = fm._rows(lambda o, b, m, *rest: L.gbwt_hip_fm_graph_positions(fm._fm, dev._h, second, o, b, m, 0, *rest), offsets, data)
        assert fm.info()["queries"] == queries + 2                               # both were computed, on the second workspace
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], flat) and np.array_equal(got_unique[1], unique)
        r_offsets, r_data = G.api._patterns_csr(c.reads)
        requests = fm.last_seed_info()["requests"]
        for most in (50, 2):
            opts = fm._seed_options(1, G.STRAND_BOTH, most)
            read_offsets, seeds, hit_offsets, hits = fm._seed_rows(lambda *a: L.gbwt_hip_fm_seed_graph_positions(fm._fm, dev._h, second, *a), r_offsets, r_data, opts)
            assert as_tuples(seeds) == [s[1:] for s in c.seeds()] and read_offsets[-1] == seeds.size
            for seed, row in zip(seeds, rows_of(hit_offsets, hits)):
                lo, hi = int(seed["lo"]), int(seed["hi"])
                assert np.array_equal(row, c.sa_tags[lo:hi] if hi - lo <= most else c.sa_tags[:0])
        assert fm.last_seed_info()["requests"] == requests + 2
        # the first workspace's later requests are unchanged
        assert np.array_equal(dev.tag_array(OTHER_IDS, np.arange(40, dtype=np.uint64)), GRAPH.tags(OTHER_IDS)[:40])
        later = fm.graph_positions_csr(patterns, unique=True)
        assert fm.info()["queries"] == queries + 3 and np.array_equal(later[1], unique)
        check_hits(fm, c.sa, c.reads, 50, values=c.sa_tags, graph=True)
    finally:
        L.gbwt_hip_workspace_destroy(second)                                     # before the handle is closed; the index before its handle
        fm.close()
