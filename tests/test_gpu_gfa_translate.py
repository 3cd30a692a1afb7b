"""Construction from GFA with a node-to-segment translation on the device (include/gbwt_hip.h, "construction from GFA with a
node-to-segment translation") against translation.gbz -- which the upstream tool made from translation.gfa with --max-node 2 --, a
pure-Python reader of the same rules (tests/gfa_translate_expect.py) and the brute-force builder (Synth.from_paths)."""
import ctypes as C
import os

import numpy as np
import pytest

import gbwt_rs_amd as G
import gfa_expect as X
import gfa_translate_expect as T
import oracle_lib as O
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S

pytestmark = pytest.mark.gpu

EXAMPLE_GFA, TRANSLATION_GFA = os.path.join(O.GOLDEN, "example.gfa"), os.path.join(O.GOLDEN, "translation.gfa")
TRANSLATION_GBZ = os.path.join(O.GOLDEN, "translation.gbz")
STATUS = {X.INVALID_DATA: _lib.INVALID_DATA, X.UNSUPPORTED: _lib.UNSUPPORTED}
COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
AUTO, ALWAYS = G.GFA_TRANSLATE_AUTO, G.GFA_TRANSLATE_ALWAYS


def reverse(s):
    return s.translate(COMPLEMENT)[::-1]


def records_of(x):
    if isinstance(x, S.Synth):
        return bytes(x.data()), list(x.starts()), (x.sequences, x.size, x.alphabet_offset, x.alphabet_size, x.bidirectional)
    data, starts = x.records()
    return bytes(data), [int(v) for v in starts], (x.sequences(), x.len(), x.alphabet_offset(), x.alphabet_size(), x.is_bidirectional())


def rows_of(dev, orientation=0):
    ids = 2 * np.arange(dev.stats.paths, dtype=np.uint64) + orientation
    offsets, nodes = dev.sequences_csr(ids)
    return [[int(v) for v in nodes[int(a):int(b)]] for a, b in zip(offsets[:-1], offsets[1:])]


def segment_rows_of(dev):
    ids = 2 * np.arange(dev.stats.paths, dtype=np.uint64)
    offsets, tokens = dev.segment_paths(ids)
    return [[int(v) for v in tokens[int(a):int(b)]] for a, b in zip(offsets[:-1], offsets[1:])]


def expected_lines(want):
    """The line gbunzip writes for every path of a translated graph: steps on segment names."""
    lines = []
    for row, (sample, contig, phase, fragment) in zip(want.segment_paths, want.names):
        names = [(want.all_segments[v // 2][0], v & 1) for v in row]
        if want.samples[sample] == "_gbwt_ref":
            lines.append(("P\t%s\t%s\t*\n" % (want.contigs[contig], ",".join(f"{n}{'-' if r else '+'}" for n, r in names))).encode("latin-1"))
        else:
            end = fragment + sum(len(want.all_segments[v // 2][1]) for v in row)
            walk = "".join(f"{'<' if r else '>'}{n}" for n, r in names)
            lines.append(f"W\t{want.samples[sample]}\t{phase}\t{want.contigs[contig]}\t{fragment}\t{end}\t{walk}\n".encode("latin-1"))
    return lines


def check_translated(dev, text, max_node, translate=AUTO, every_label=True):
    """Rows, records, segments, labels, names and counters of a built handle are what the text says."""
    if isinstance(text, str):
        text = text.encode()
    want = T.Translated(text, max_node, translate)
    assert want.translated
    assert dev.stats.is_gbz == 1 and dev.stats.has_metadata == 1 and dev.stats.has_translation == 1 and dev.stats.paths == len(want.paths)
    assert rows_of(dev) == want.paths
    assert (dev.alphabet_offset(), dev.alphabet_size()) == (1, 2 * want.total_nodes + 2)               # one slot per node, visited or not
    visited_nodes = {v // 2 for row in want.paths for v in row}
    if {1, want.total_nodes} <= visited_nodes:                                                        # (the brute-force builder sizes its alphabet by the visits)
        assert records_of(dev) == records_of(S.Synth.from_paths(want.paths, bidirectional=True))
    assert segment_rows_of(dev) == want.segment_paths
    visited = [row[0] for row in want.segments if row[1]]
    assert [int(v) for v in dev.segment_iter()] == visited
    nodes = np.arange(0, want.total_nodes + 2, dtype=np.uint64)
    segs, valid = dev.node_to_segments(nodes)
    for row in want.segments:
        inside = slice(row[2], row[3])
        assert valid[inside].all() == bool(row[1]) and valid[inside].any() == bool(row[1]), row[:4]
        if row[1]:
            assert (segs[inside] == row[0]).all(), row[:4]
    assert not valid[0] and not valid[want.total_nodes + 1]
    for v, label in (want.node_labels.items() if every_label else []):                                # the label of every node: a chunk of its segment
        assert dev.node_sequence(v) == (label if label else None), v
    assert dev.node_sequence(0) is None and dev.node_sequence(want.total_nodes + 1) is None
    for k, line in enumerate(expected_lines(want)):
        assert dev.path_lines([k], 1 if line[:1] == b"W" else 0) == line, k
    s_lines = [line for line in dev.graph_lines().split(b"\n") if line[:1] == b"S"]
    assert s_lines == [f"S\t{row[1]}\t{row[4]}".encode("latin-1") for row in want.segments if row[1]]
    info, tr, build = dev.last_gfa_info(), dev.last_gfa_translation_info(), dev.last_build_info()
    assert (info["bytes"], info["steps"], info["p_lines"] + info["w_lines"], info["segments"]) == (len(text), want.steps, len(want.paths), len(want.segments))
    assert (tr["translated"], tr["segments"], tr["nodes"]) == (1, len(want.segments), want.total_nodes)
    assert tr["chopped_segments"] == sum(row[3] - row[2] > 1 for row in want.segments) and tr["unvisited_segments"] == len(want.segments) - len(visited)
    assert tr["name_bytes"] == sum(len(row[1]) for row in want.segments) and tr["table_bytes"] >= 24 * len(want.segments)
    assert build["built"] == 1 and build["visits"] == 2 * sum(len(row) for row in want.paths)
    return want


def build_checked(text, max_node, translate=AUTO, **kw):
    if isinstance(text, str):
        text = text.encode("latin-1")
    dev = G.GBZ.from_gfa_text(text, max_node=max_node, translate=translate)
    return dev, check_translated(dev, text, max_node, translate, **kw)


def refused(text, line, status=X.INVALID_DATA, max_node=2, translate=AUTO):
    if isinstance(text, str):
        text = text.encode("latin-1")
    with pytest.raises(X.Refused) as expected:                # the contract, read by the reader of the expected values
        T.Translated(text, max_node, translate)
    assert (expected.value.line, expected.value.status) == (line, status)
    h = C.c_void_p(1)
    opts = _lib.GfaOptions(max_node, translate)
    got = _lib.lib().gbwt_hip_build_from_gfa_text_opts(text, len(text), C.byref(opts), 0, _lib.OPEN_ALL, C.byref(h))
    message = _lib.lib().gbwt_hip_last_error().decode()
    assert got == STATUS[status] and f"line {line}:" in message, (got, message)
    assert not h.value


@pytest.fixture(scope="module")
def tile():
    return G.parse_gfa(EXAMPLE_GFA)["tile_bytes"]


def pad(n):
    """n bytes of lines that a construction ignores"""
    out = []
    while n > 0:
        k = min(n, 61)
        if n - k == 1:
            k -= 1
        out.append("#" * (k - 1) + "\n")
        n -= k
    return "".join(out)


# ---- 1. the fixture the upstream tool made ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def loaded():
    return G.GBZ.load(TRANSLATION_GBZ)


def same_graph(dev, ref):
    """Every segment and link query answers as for `ref`."""
    assert records_of(dev) == records_of(ref)
    ids = np.arange(ref.stats.paths, dtype=np.uint64)
    for mode in (0, 1, 2):
        assert dev.path_lines(ids, mode) == ref.path_lines(ids, mode)
    assert np.array_equal(dev.segment_iter(), ref.segment_iter())
    nodes = np.arange(0, ref.alphabet_size() // 2 + 2, dtype=np.uint64)
    for a, b in zip(dev.node_to_segments(nodes), ref.node_to_segments(nodes)):
        assert np.array_equal(a, b)
    for v in nodes:
        assert dev.node_sequence(v) == ref.node_sequence(v), v
    n_segments = int(ref.segment_iter().max()) + 1
    segments = np.repeat(np.arange(n_segments, dtype=np.uint64), 2)
    orientations = np.tile(np.array([0, 1], dtype=np.uint8), n_segments)
    for predecessors in (False, True):
        for a, b in zip(dev.links_csr(segments, orientations, predecessors), ref.links_csr(segments, orientations, predecessors)):
            assert np.array_equal(a, b)
    sequences = np.arange(2 * ref.stats.paths, dtype=np.uint64)
    for a, b in zip(dev.segment_paths(sequences), ref.segment_paths(sequences)):
        assert np.array_equal(a, b)
    assert dev.graph_lines() == ref.graph_lines()


def test_fixture(loaded, tmp_path):
    dev = G.GBZ.from_gfa(TRANSLATION_GFA, max_node=2, translate=AUTO)
    want = check_translated(dev, open(TRANSLATION_GFA, "rb").read(), 2)
    assert want.segments[4] == [4, "", 7, 9, ""]
    same_graph(dev, loaded)
    loaded.write_gfa(str(tmp_path / "loaded.gfa"))
    dev.write_gfa(str(tmp_path / "built.gfa"))
    assert (tmp_path / "built.gfa").read_bytes() == (tmp_path / "loaded.gfa").read_bytes()
    dev.save(str(tmp_path / "built.gbz"))
    assert O.OracleGBZ(str(tmp_path / "built.gbz")).gfa() == O.OracleGBZ(TRANSLATION_GBZ).gfa()
    again = G.GBZ.load(str(tmp_path / "built.gbz"))
    assert again.stats.has_translation == 1
    same_graph(again, loaded)
    assert set(loaded.last_gfa_translation_info().values()) == {0}          # a handle that was not made from GFA


def test_translation_gfa_without_options_is_still_unsupported():
    with pytest.raises(G.GbwtHipError) as e:
        G.GBZ.from_gfa(TRANSLATION_GFA)
    assert e.value.status == _lib.UNSUPPORTED and "line 2:" in str(e.value) and "translation" in str(e.value)
    h = C.c_void_p(1)
    text = open(TRANSLATION_GFA, "rb").read()
    for opts in (None, C.byref(_lib.GfaOptions(0, G.GFA_TRANSLATE_NEVER))):
        assert _lib.lib().gbwt_hip_build_from_gfa_text_opts(text, len(text), opts, 0, _lib.OPEN_ALL, C.byref(h)) == _lib.UNSUPPORTED
        assert "line 2:" in _lib.lib().gbwt_hip_last_error().decode() and not h.value


# ---- 2. fixed points ---------------------------------------------------------------------------------------------------------------------------

def test_gbunzip_of_the_fixture_is_a_fixed_point(loaded, tmp_path):
    out = tmp_path / "t.gfa"
    loaded.write_gfa(str(out))
    text = out.read_bytes()
    for _ in range(2):
        dev = G.GBZ.from_gfa(str(out), max_node=2)
        check_translated(dev, text, 2)
        dev.write_gfa(str(out))
        assert out.read_bytes() == text


def test_example_with_names_for_its_ids(tmp_path):
    dev = G.GBZ.from_gfa(EXAMPLE_GFA, max_node=0, translate=ALWAYS)
    want = check_translated(dev, open(EXAMPLE_GFA, "rb").read(), 0, ALWAYS)
    assert [(row[1], row[2]) for row in want.segments] == [(str(v), k + 1) for k, v in enumerate((11, 12, 13, 14, 15, 16, 17, 21, 22, 23, 24, 25))]
    G.GBZ.load(os.path.join(O.GOLDEN, "example.gbz")).write_gfa(str(tmp_path / "gbunzip.gfa"))
    dev.write_gfa(str(tmp_path / "built.gfa"))
    assert (tmp_path / "built.gfa").read_bytes() == (tmp_path / "gbunzip.gfa").read_bytes()


def test_auto_falls_through():
    plain = G.GBZ.from_gfa(EXAMPLE_GFA)
    for dev in (G.GBZ.from_gfa(EXAMPLE_GFA, max_node=1024, translate=AUTO), G.GBZ.from_gfa(EXAMPLE_GFA, max_node=1), G.GBZ.from_gfa(EXAMPLE_GFA, translate=AUTO)):
        assert records_of(dev) == records_of(plain) and dev.stats.has_translation == 0
        for v in range(10, 27):
            assert dev.node_sequence(v) == plain.node_sequence(v), v
        tr = dev.last_gfa_translation_info()
        assert tr["translated"] == 0 and tr["nodes"] == 0 and tr["segments"] == 12
        assert dev.last_gfa_info()["steps"] == plain.last_gfa_info()["steps"] == 28


# ---- 3. chopping --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 1024])
def test_chopping_edges(m):
    rng = np.random.default_rng(m)
    lengths = sorted({max(1, m - 1), m, m + 1, 2 * m, 2 * m + 1}) + [70000]
    labels = {f"seg{k}": bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)) for k, n in enumerate(lengths)}
    names = list(labels)
    text = b"".join(b"S\t%s\t%s\n" % (name.encode(), s) for name, s in labels.items())
    text += ("W\ts\t1\tc\t0\t1\t" + "".join(f"{'<' if k % 2 else '>'}{name}" for k, name in enumerate(names)) + "\n").encode()
    text += ("P\tp\t" + ",".join(f"{name}{'+' if k % 2 else '-'}" for k, name in enumerate(reversed(names))) + "\n").encode()
    dev, want = build_checked(text, m)
    assert [row[3] - row[2] for row in want.segments] == [max(1, -(-n // m)) for n in lengths]
    for row in want.segments:                                  # every node but a segment's last carries exactly m bytes
        sizes = [len(want.node_labels[v]) for v in range(row[2], row[3])]
        assert sizes[:-1] == [m] * (len(sizes) - 1) and 1 <= sizes[-1] <= m and sum(sizes) == len(row[4])
    offsets, bases = dev.path_sequences([0, 1])
    p_row = b"".join(labels[name] if k % 2 else reverse(labels[name]) for k, name in enumerate(reversed(names)))
    w_row = b"".join(reverse(labels[name]) if k % 2 else labels[name] for k, name in enumerate(names))
    assert bytes(bases) == p_row + w_row and [int(v) for v in offsets] == [0, len(p_row), len(p_row) + len(w_row)]


# ---- 4. tile edges ------------------------------------------------------------------------------------------------------------------------------

LONG = "n" * 255
HEAD = f"S\ta+b\tACG\nS\t{LONG}\tGT\nS\tx-\tTTTTT\nS\t7\tC\n"
P_LINE = f"P\tp\ta+b+,{LONG}-,x--,7+\t*\n"
W_LINE = f"W\ts\t1\tc\t0\t9\t>a+b<{LONG}>x-<7\n"
EDGE_BYTES = {
    "p-first-token": (P_LINE, P_LINE.index("a+b")),
    "p-token-start": (P_LINE, P_LINE.index(LONG)),
    "p-name-byte": (P_LINE, P_LINE.index(LONG) + 100),
    "p-long-name-last-byte": (P_LINE, P_LINE.index(LONG) + 254),
    "p-orientation": (P_LINE, P_LINE.index(LONG) + 255),
    "p-comma": (P_LINE, P_LINE.index(LONG) + 256),
    "p-orientation-behind-a-minus": (P_LINE, P_LINE.index("x--") + 2),
    "w-token-start": (W_LINE, W_LINE.index("<" + LONG)),
    "w-name-byte": (W_LINE, W_LINE.index(LONG) + 100),
    "w-long-name-last-byte": (W_LINE, W_LINE.index(LONG) + 254),
    "w-next-mark": (W_LINE, W_LINE.index(">x-")),
}


@pytest.mark.parametrize("what", sorted(EDGE_BYTES))
def test_byte_at_a_tile_edge(what, tile):
    line, index = EDGE_BYTES[what]
    tail = "W\ts\t2\tc\t0\t1\t<x-\nP\tq\t7-\n"
    for edge in (tile, 2 * tile):
        for at in (edge - 1, edge, edge + 1):
            text = HEAD + pad(at - index - len(HEAD)) + line + tail
            assert text.index(line) + index == at
            build_checked(text, 2)


def test_long_walk_between_short_ones(tile):
    names = ["a+b", LONG[:9], "x-", "7"]
    head = HEAD.replace(LONG, LONG[:9])
    steps = 3 * tile // 4 + 1
    walk = "".join(f"{'<' if k % 3 == 0 else '>'}{names[k % 4]}" for k in range(steps))
    assert len(walk) > 3 * tile
    text = head + f"W\ts\t1\tc\t0\t1\t>a+b\nW\ts\t2\tc\t0\t1\t{walk}\nW\ts\t3\tc\t0\t1\t<x-\nP\tp\t7+\nW\ts\t4\tc\t0\t1\t>7\n"
    dev, want = build_checked(text, 2)
    assert [len(p) for p in want.segment_paths] == [1, 1, steps, 1, 1]


# ---- 5. names -----------------------------------------------------------------------------------------------------------------------------------

def test_many_names(tmp_path):
    rng = np.random.default_rng(11)
    alphabet = np.frombuffer(b"abcXYZ0123456789+-._#*:", dtype=np.uint8)
    names = ["3", "1", "12", "4999", "+", "-", "+-", "1+", "-1", "a", "a+", "a+-"]    # decimal ids of other segments' nodes; orientation bytes; prefixes of one another
    seen = set(names)
    while len(names) < 5000:
        name = bytes(rng.choice(alphabet, size=int(rng.integers(1, 41)))).decode()
        if name not in seen and name != "*":
            seen.add(name)
            names.append(name)
    order = [int(v) for v in rng.permutation(len(names))]
    names = [names[k] for k in order]
    sequences = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(1, 9)))).decode() for _ in names]
    unvisited = {0, 2500, 4999}
    steps = [int(v) for v in rng.integers(0, 5000, size=6000) if int(v) not in unvisited]
    special = [k for k, name in enumerate(names) if len(name) <= 3 and k not in unvisited]
    p_steps, w_steps = special + steps[:3000], steps[3000:] + special
    text = "".join(f"S\t{name}\t{seq}\n" for name, seq in zip(names, sequences))
    text += "P\tp\t" + ",".join(f"{names[k]}{'-' if k % 3 == 0 else '+'}" for k in p_steps) + "\n"
    text += "W\ts\t1\tc\t0\t1\t" + "".join(f"{'<' if k % 5 == 0 else '>'}{names[k]}" for k in w_steps) + "\n"
    dev, want = build_checked(text, 3)
    assert [row[1] for row in want.segments if row[0] in unvisited] == ["", "", ""] and want.segments[0][2:4] == [1, 1 + -(-len(sequences[0]) // 3)]
    assert dev.node_sequence(1) is None and dev.node_sequence(want.total_nodes) is None
    dev.save(str(tmp_path / "names.gbz"))                      # an unvisited segment first and last: the file still loads, and says the same
    again = G.GBZ.load(str(tmp_path / "names.gbz"))
    assert records_of(again) == records_of(dev) and again.graph_lines() == dev.graph_lines()
    assert rows_of(again) == want.paths and segment_rows_of(again) == want.segment_paths
    oracle = O.OracleGBZ(str(tmp_path / "names.gbz"))
    dev.write_gfa(str(tmp_path / "names.gfa"))
    assert oracle.gfa() == (tmp_path / "names.gfa").read_bytes()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------

GOOD = "S\ta\tACG\nS\tb\tC\nS\t3\tG\n"
REFUSALS = {
    "duplicate-name": (GOOD + "S\tc\tT\nS\tb\tT\nP\tp\ta+\n", 5, X.INVALID_DATA),
    "duplicate-name-three-times": ("S\tb\tT\n#\nS\tb\tT\nS\tb\tT\n", 3, X.INVALID_DATA),
    "name-of-256-bytes": (GOOD + "S\t" + "n" * 256 + "\tT\n", 4, X.UNSUPPORTED),
    "empty-name": (GOOD + "S\t\tT\n", 4, X.INVALID_DATA),
    "unknown-name-p": (GOOD + "#\nP\tp\ta+,d-\n", 5, X.INVALID_DATA),
    "unknown-name-w": (GOOD + "W\ts\t1\tc\t0\t1\t>a>d\n", 4, X.INVALID_DATA),
    "unknown-name-that-is-a-node-id": (GOOD + "P\tp\ta+,2+\n", 4, X.INVALID_DATA),
    "unknown-name-of-300-bytes-p": (GOOD + "P\tp\ta+," + "n" * 300 + "+\n", 4, X.INVALID_DATA),
    "unknown-name-of-300-bytes-w": (GOOD + "W\ts\t1\tc\t0\t1\t>a>" + "n" * 300 + "\n", 4, X.INVALID_DATA),
    "empty-token-p": (GOOD + "P\tp\ta+,,b+\n", 4, X.INVALID_DATA),
    "empty-token-w": (GOOD + "W\ts\t1\tc\t0\t1\t>a>>b\n", 4, X.INVALID_DATA),
    "empty-token-at-the-end-w": (GOOD + "W\ts\t1\tc\t0\t1\t>a>\n", 4, X.INVALID_DATA),
    "trailing-comma": (GOOD + "P\tp\ta+,\n", 4, X.INVALID_DATA),
    "leading-comma": (GOOD + "P\tp\t,a+\n", 4, X.INVALID_DATA),
    "p-token-without-orientation": (GOOD + "P\tp\ta+,b\n", 4, X.INVALID_DATA),
    "p-token-that-is-only-an-orientation": (GOOD + "P\tp\ta+,+\n", 4, X.INVALID_DATA),
    "walk-without-a-first-mark": (GOOD + "W\ts\t1\tc\t0\t1\ta>b\n", 4, X.INVALID_DATA),
    "s-with-a-star": (GOOD + "S\tc\t*\n", 4, X.INVALID_DATA),
    "carriage-return": (GOOD + "P\tp\ta+\t*\r\n", 4, X.INVALID_DATA),
    "non-numeric-haplotype": (GOOD + "W\ts\tone\tc\t0\t1\t>a\n", 4, X.INVALID_DATA),
    "duplicate-path-name": (GOOD + "W\ts\t1\tc\t0\t1\t>a\n#\nW\ts\t1\tc\t*\t1\t>b\n", 6, X.INVALID_DATA),
    "two-bad-lines-step-first": (GOOD + "P\tp\ta+,d+\nS\t" + "n" * 256 + "\tA\n", 4, X.INVALID_DATA),
    "two-bad-lines-name-first": (GOOD + "S\t" + "n" * 256 + "\tA\nP\tp\ta+,d+\n", 4, X.UNSUPPORTED),
    "two-bad-lines-duplicate-first": (GOOD + "S\ta\tA\nW\ts\t1\tc\t0\t1\t>a>>b\n", 4, X.INVALID_DATA),
    "two-bad-lines-token-first": (GOOD + "W\ts\t1\tc\t0\t1\t>a>>b\nS\ta\tA\n", 4, X.INVALID_DATA),
    "two-bad-lines-host-first": (GOOD + "W\ts\tone\tc\t0\t1\t>a\nP\tp\ta+,d+\n", 4, X.INVALID_DATA),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(name):
    refused(*REFUSALS[name])


def test_names_with_orientation_bytes_are_not_refused():
    build_checked(GOOD + "S\tb+\tTT\nS\t-\tA\nP\tp\tb++,--,b+,3-\nW\ts\t1\tc\t0\t1\t>b+<->b<3\n", 2)
