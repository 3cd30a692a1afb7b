"""What tests/test_gpu_fm_paths.py relies on, pinned without a GPU: the texts, bounds and tags that tests/fm_path_graphs.py derives from its
own labels and walks are those the existing yardsticks (seq_expect, tags_expect) give for a golden GFA; the graphs have the shapes they are
built for; the figures of the periodic graph hold; and every case holds the seeds, chains and windows that make a pass on the GPU mean
something."""
import os

import numpy as np
import pytest

import chain_expect as X
import fm_expect as F
import fm_path_graphs as P
import oracle_lib as O
import seed_expect as E
import seq_expect as Q
import shifted_graphs as SG
import tags_expect as T

MOST = 1 << 20
GRAPH = P.tangle_small()
ORDERS = P.orders(GRAPH)
PERIODIC = dict(min_length=5, strands=E.FORWARD, max_occurrences=MOST, max_gap=400, max_skew=8)


@pytest.fixture(scope="module", params=[(name, e) for name in P.ORDER_NAMES for e in P.ENDMARKERS], ids=lambda p: f"{p[0]}-{p[1]}")
def case(request):
    name, e = request.param
    return name, P.Case(GRAPH, ORDERS[name], e)


def test_text_and_tags_of_a_golden_gfa_are_those_of_the_existing_yardsticks():
    gfa = open(os.path.join(O.GOLDEN, "example.gfa"), "rb").read()
    g = P.from_gfa(gfa)
    rows = T.gfa_rows(gfa)
    table = Q.LabelTable.from_gfa(gfa)
    assert g.paths() == len(rows) == 6
    for order in (list(range(6)), [5, 0, 3], [2, 2, 4, 2], [4]):
        for endmarker in (0, 36, 65):
            node_rows = [(rows[p].astype(np.int64) >> 1, (rows[p] & np.uint64(1)).astype(bool)) for p in order]
            offsets, data = Q.expected_rows(table, node_rows, endmarker)
            assert g.text(order, endmarker) == data and g.bounds(order) == offsets.tolist()
        tags, offsets = T.tag_text(table.len, [rows[p] for p in order])
        assert np.array_equal(g.tags(order), tags) and g.bounds(order) == offsets.tolist()
    # by hand: the walk >21>22>24<23<21 reads G A T, then T reversed (A) and G reversed (C), on node 21 in reverse at last
    assert g.row_text(4) == b"GATAC" and g.tags([4]).tolist() == [21 << 11, 22 << 11, 24 << 11, (23 << 11) | (1 << 10), (21 << 11) | (1 << 10), 0]
    assert g.step_starts(4) == [0, 1, 2, 3, 4] and g.visits([0, 4], 21, 1) == [(1, 4)]
    # the GFA text the helper writes is W-lines only and reads back as itself
    again = P.from_gfa(g.gfa())
    assert again.labels == g.labels and again.walks == g.walks and b"\nP\t" not in g.gfa() and g.gfa().count(b"\nW\t") == 6


def test_the_tangle_is_what_it_is_built_for():
    g = GRAPH
    lengths = sorted(len(label) for label in g.labels.values())
    assert len(g.labels) == 40 and set(lengths) == {1, 2, 15, 16, 17, 31, 33, 200} and lengths.count(200) == 1
    assert {v for walk in g.walks for v, _ in walk} == set(g.labels)                       # every node is on a path: none is dropped by the build
    assert [len(walk) for walk in g.walks] == [13, 1, 26, 2, 26, 3, 39, 13]
    steps = [step for walk in g.walks for step in walk]
    assert 0.25 < sum(o for _, o in steps) / len(steps) < 0.35
    pairs = [(a, b) for walk in g.walks for a, b in zip(walk[:-1], walk[1:])]
    assert any(a == b for a, b in pairs) and any(a[0] == b[0] and a[1] != b[1] for a, b in pairs)        # x x, and x rev(x)
    assert any(len({v for v, _ in walk}) < len(walk) - 2 for walk in g.walks)              # revisits beyond the immediate ones
    assert g.visits(range(8), P.LONG_NODE, 0) and g.visits(range(8), P.LONG_NODE, 1)
    assert g.walks[0] == g.walks[7] and g.row_text(0) == g.row_text(7)
    assert g.walks[4] == P.reversed_walk(g.walks[2]) and g.row_text(4) == P.reverse_complement(g.row_text(2))
    assert g.walks[P.ONE_STEP_PATH] == [(1, 0)] and len(g.text([P.ONE_STEP_PATH])) == 2
    assert len(set(g.gfa().split(b"\n"))) == len(g.gfa().split(b"\n"))                     # no two lines are equal: the W-lines of equal walks differ
    for name, order in ORDERS.items():
        assert len(g.text(order)) == g.bounds(order)[-1] <= 3000, name
    assert ORDERS["subset"] == [0, 2, 4, 6, 1] and ORDERS["duplicate"][-2:] == [7, 0]


def test_shifted_tangle_text_moves_only_the_names():
    g, gfa = GRAPH, GRAPH.gfa()
    for shift, d in SG.SHIFTS(P.LONG_NODE).items():
        moved = P.from_gfa(SG.shift_gfa(gfa, d))
        assert sorted(moved.labels) == [v + d for v in sorted(g.labels)] and all(moved.labels[v + d] == label for v, label in g.labels.items())
        assert moved.walks == [[(v + d, o) for v, o in walk] for walk in g.walks]
        assert [moved.row_text(p) for p in range(8)] == [g.row_text(p) for p in range(8)]
    tags = g.tags(range(8))
    top = SG.move_tags(tags, SG.SHIFTS(P.LONG_NODE)["top"])
    assert int(top.max()) > 1 << 41 and int(np.count_nonzero(top == 0)) == 8 == int(np.count_nonzero(tags == 0))
    assert int(top.max()) == (SG.MAX_NODE_ID << 11) + (1 << 10) + 199                     # the last base of the long node, read in reverse


def test_conditions_that_keep_the_gpu_cases_honest(case):
    name, c = case
    assert len(c.reads) <= 200 and len(c.text) <= 3000
    assert c.reads_without_seeds(), name                                                   # a read of bytes the text lacks on both strands
    across = c.seeds_over_a_path_end()
    if name == "single":
        # one segment of one base and its endmarker: no seed has hits in two segments, no chain has two members, no read runs over an end
        assert len(c.text) == 2 and not c.seeds_in_two_segments() and not across
        return
    assert c.seeds_in_two_segments(), name
    want = X.expected_rows(c.text, c.sa, c.reads, 4, E.BOTH, MOST, 1000, 50, bounds=c.bounds)
    assert any(row[5] >= 2 for row in want["chains"]), name
    assert len({row[7] for row in want["chains"]}) > 1
    if name == "reversed":                                                                 # the bases of two long paths as one read: an item larger than the DP's tile of 512
        assert max(len(X.matches_of(c.text, c.sa, read, strand, 4)) for read in c.reads[-20:] for strand in (E.FORWARD, E.REVERSE)) > 700
    # the reads with the endmarker byte between the flanks occur as a whole: their seed runs through a path's end
    assert across and all(c.text[p + s[2] - s[1] - 1:].find(bytes([c.endmarker])) >= 0 for s, p in across)
    if c.endmarker == 65:
        assert any(65 in c.reads[s[0]] and 0 not in c.reads[s[0]] for s, _ in across)      # ... with a literal A in the gap


def test_chains_of_a_path_named_twice_come_once_per_copy():
    """What the duplicate case asserts on the device's rows, held on the yardstick's: segments 7 and 8 of the list hold path 7 twice."""
    c = P.Case(GRAPH, ORDERS["duplicate"], 0)
    assert c.order[7] == c.order[8] == 7
    want = X.expected_rows(c.text, c.sa, c.reads, 4, E.BOTH, MOST, 1000, 50, bounds=c.bounds)
    distance = c.bounds[8] - c.bounds[7]
    first = sorted((k,) + row for k in range(len(c.reads)) for row in want["chains"][want["read_offsets"][k]:want["read_offsets"][k + 1]] if row[7] == 7)
    second = sorted((k,) + row for k in range(len(c.reads)) for row in want["chains"][want["read_offsets"][k]:want["read_offsets"][k + 1]] if row[7] == 8)
    assert first and [(r[0], r[1] + distance, r[2] + distance) + r[3:8] + (8,) for r in first] == second


def periodic_item(reps, endmarker=0):
    g = P.periodic(reps)
    order = list(range(len(reps)))
    text, bounds = g.text(order, endmarker), g.bounds(order)
    assert text == b"".join(b"AC" * r + bytes([endmarker]) for r in reps) and len(text) <= 3000
    sa = F.suffix_array(text)
    return text, bounds, sa, X.matches_of(text, sa, P.PERIODIC_READ, E.FORWARD, 5)


@pytest.mark.parametrize("reps,count", [([120, 3, 2, 70, 74], 518), ([40, 30], 132), ([120, 3, 2, 70, 71], 512), ([120, 3, 2, 70, 72], 514)])
def test_periodic_match_counts(reps, count):
    _, _, _, matches = periodic_item(reps)
    assert len(matches) == count == P.periodic_matches(reps)
    assert {m[1:] for m in matches} == {(0, 6), (7, 6)}
    if reps[0] == 120:
        assert P.periodic_reps_for(count) == reps


def test_periodic_figures_with_and_without_bounds():
    reps = [120, 3, 2, 70, 74]
    text, bounds, sa, matches = periodic_item(reps)
    cut = X.expected_rows(text, sa, [P.PERIODIC_READ], bounds=bounds, **PERIODIC)
    plain = X.expected_rows(text, sa, [P.PERIODIC_READ], **PERIODIC)
    assert (cut["n_matches"], cut["pairs"], len(cut["chains"])) == (518, 1722, 269)
    assert (plain["n_matches"], plain["pairs"], len(plain["chains"])) == (518, 1744, 266)
    assert all(bounds[row[7]] <= row[0] and row[1] <= bounds[row[7] + 1] - 1 for row in cut["chains"])
    assert any(any(row[0] < b <= row[1] - 1 for b in bounds[1:-1]) for row in plain["chains"])
    assert sorted({row[7] for row in cut["chains"]}) == [0, 1, 3, 4]                       # the 2-repeat path has no match


@pytest.mark.parametrize("reps", [[120, 3, 2, 70, 71], [120, 3, 2, 70, 72], [40, 30]])
def test_periodic_dp_equals_the_definition_in_loops(reps):
    _, bounds, _, matches = periodic_item(reps)
    y, x, w = ([m[k] for m in matches] for k in range(3))
    opts = X.options(400, 8)
    for b in (bounds, None):
        seg = X.segments(y, b)
        assert X.dp(y, x, w, seg, opts) == X.dp_slow(y, x, w, seg.tolist(), opts)


@pytest.mark.parametrize("reps", [[120, 3, 2, 70, 71], [120, 3, 2, 70, 72], [40, 30]])
def test_periodic_windows_are_wider_than_two_waves_and_jump(reps):
    _, bounds, _, matches = periodic_item(reps)
    sizes, starts = P.window_sizes(matches, bounds, 400), P.window_starts(matches, bounds, 400)
    jumps = np.diff(starts)
    if reps[0] == 120:
        assert sizes.max() > 128 and jumps.max() > 128                                     # the first match of path 1 leaves the 236 of path 0 behind
        assert int(starts[int(jumps.argmax()) + 1]) == 236
    else:
        assert 64 < sizes.max() <= 128 and jumps.max() > 64                                # one chunk and a part; the second path skips the 76 of the first
    assert (jumps >= 0).all()


def test_segments_with_repeated_bounds_pick_the_last_index():
    assert X.segments([0, 4, 5, 8], [0, 5, 5, 9]).tolist() == [0, 0, 2, 2]
    assert X.segments([0, 1, 2], [0, 0, 0, 3]).tolist() == [2, 2, 2]
    assert X.segments([7, 3], None).tolist() == [0, 0]
    bounds = GRAPH.bounds(ORDERS["duplicate"])
    assert X.segments([bounds[9], bounds[9] - 1, bounds[10] - 1], bounds).tolist() == [9, 8, 9]
