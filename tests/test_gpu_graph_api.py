"""The graph API on the device -- node ids, edge rows, segments, link rows, and the H-, S- and L-lines of a GFA file -- against
tests/graph_expect.py (the oracle's records and GFA; pinned on the CPU in tests/test_graph_expect_cpu.py): the golden files, the graphs of
tests/tangled_graphs.py (a record of 5 000 edges, self-loops and reverse joins, slots without nodes, a unidirectional index), rows around
the hand-off to a workgroup, labels of 1 to 70 000 bases and of the largest accepted length, a synthetic translation, and the plumbing."""
import ctypes as C
import os

import numpy as np
import pytest

import gbwt_rs_amd as G
import graph_expect as X
import oracle_lib as O
import tangled_graphs as TG
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S

pytestmark = pytest.mark.gpu

LARGEST_LABEL = 4194299                          # the longest label the bases kernel accepts (tests/test_gpu_tangled.py)
NEEDS_GFA = "need a GBZ opened with GBWT_HIP_OPEN_GFA"


def both_orientations(ids):
    ids = np.asarray(ids, dtype=np.uint64)
    return np.repeat(ids, 2), np.tile(np.array([0, 1], dtype=np.uint8), ids.size)


def check_rows(got, rows):
    offsets, flat, valid = got
    e_off, e_flat, e_valid = X.csr(rows)
    assert offsets.dtype == np.uint64 and flat.dtype == np.uint64
    assert np.array_equal(valid, e_valid)
    assert np.array_equal(offsets, e_off)
    assert np.array_equal(flat, e_flat)


def check_edges(dev, graph, ids, orient):
    """successors and predecessors of every (id, orientation), each direction in one call."""
    for predecessors in (False, True):
        rows = [graph.edges(int(i), int(o), predecessors) for i, o in zip(ids, orient)]
        check_rows(dev.edges_csr(ids, orient, predecessors), rows)


def check_links(dev, translation, ids, orient):
    for predecessors in (False, True):
        rows = [translation.links(int(i), int(o), predecessors) for i, o in zip(ids, orient)]
        check_rows(dev.links_csr(ids, orient, predecessors), rows)


def mixed_request(graph, seed):
    """A shuffled request with duplicates and ids that are no nodes: 0, below min_node, slots without nodes, past the alphabet, huge."""
    rng = np.random.default_rng(seed)
    real = np.array(graph.node_ids(), dtype=np.uint64)
    ids = np.concatenate([rng.choice(real, size=min(real.size, 3000)), rng.choice(real, size=50).repeat(3),
                          rng.integers(0, graph.max_node + 3, size=500).astype(np.uint64),
                          np.array([0, graph.max_node + 1, graph.max_node + 2, 1 << 40, (1 << 62) - 1, 1 << 62, (1 << 64) - 1], dtype=np.uint64)])
    ids = ids[rng.permutation(ids.size)]
    return ids, rng.integers(0, 2, size=ids.size).astype(np.uint8)


def check_graph_text(dev, oracle, tmp_path):
    """graph_lines() = the H-, S- and L-lines of the oracle = the head of the file write_gfa of this build writes."""
    gfa = oracle.gfa()
    want = X.graph_text(gfa)
    got = dev.graph_lines()
    assert len(got) == len(want)
    assert got == want
    out = tmp_path / "whole.gfa"
    dev.write_gfa(str(out))
    assert out.read_bytes()[: len(got)] == got
    text = dev.graph_lines_device()
    assert text.header_bytes + text.segment_bytes + text.link_bytes == len(want)
    assert (text.header_bytes, text.segment_bytes, text.link_bytes) == tuple(len(X.lines_of(gfa, k)) for k in (b"H", b"S", b"L"))
    assert (text.segments, text.links) == (want.count(b"\nS\t"), want.count(b"\nL\t"))
    return want


# ---- the golden files ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["example.gbz", "translation.gbz"])
def test_golden_gbz(tmp_path, name):
    path = os.path.join(O.GOLDEN, name)
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    graph = X.Graph(oracle.gbwt())
    ids, orient = both_orientations(np.arange(0, graph.max_node + 3))
    check_edges(dev, graph, ids, orient)
    assert dev.node_iter().tolist() == graph.node_ids()
    known = X.known()[name]
    for key, predecessors in (("successors", False), ("predecessors", True)):
        for case in known.get(key, []):
            one = dev.predecessors(case["node"], case["orientation"]) if predecessors else dev.successors(case["node"], case["orientation"])
            assert one == [tuple(e) for e in case["edges"]]
    assert dev.successors(0, 0) is None and dev.predecessors(graph.max_node + 1, 1) is None
    check_graph_text(dev, oracle, tmp_path)
    all_nodes = np.arange(0, graph.max_node + 3, dtype=np.uint64)
    if name == "translation.gbz":
        assert dev.has_translation()
        t = X.Translation(graph, [row[:4] for row in known["segments"]])
        seg_ids, seg_orient = both_orientations(np.arange(0, len(t.segments) + 2))
        check_links(dev, t, seg_ids, seg_orient)
        assert dev.segment_iter().tolist() == t.segment_ids()
        got, valid = dev.node_to_segments(all_nodes)
        want = [t.node_to_segment(int(v)) for v in all_nodes]
        assert valid.tolist() == [w is not None for w in want] and got[valid].tolist() == [w for w in want if w is not None]
        by_name = {row[1]: row[0] for row in known["segments"] if row[1]}
        assert dev.segment_successors(by_name["s14"], 0) == [(by_name["s15"], 0), (by_name["s16"], 0)]
        assert dev.segment_predecessors(by_name["s11"], 1) == [(by_name["s12"], 1), (by_name["s13"], 1)]
        assert dev.node_to_segment(5) == by_name["s14"] and dev.node_to_segment(7) is None
        assert dev.segment_successors(4, 0) is None and dev.segment_successors(len(t.segments), 1) is None
    else:
        assert not dev.has_translation() and dev.segment_iter() is None and dev.node_to_segment(24) is None
        offsets, links, valid = dev.links_csr([0, 1, 2], [0, 1, 0])
        assert not valid.any() and links.size == 0 and offsets.tolist() == [0, 0, 0, 0]


def test_golden_bare_gbwt_answers_edges_and_refuses_links_and_lines():
    path = os.path.join(O.GOLDEN, "example.gbwt")
    dev = G.GBZ.load(path)                        # (the GBZ mirror over a bare GBWT: its graph calls must refuse)
    graph = X.Graph(O.OracleGBWT.load(path))
    ids, orient = both_orientations(np.arange(0, graph.max_node + 3))
    check_edges(dev, graph, ids, orient)
    assert dev.node_iter().tolist() == graph.node_ids()
    lean = G.GBWT.load(path, flags=_lib.OPEN_EXTRACT)
    check_edges(lean, graph, ids, orient)
    for call in (lambda: dev.links_csr([0], [0]), dev.graph_lines, dev.graph_lines_device, lambda: dev.node_to_segments([11])):
        with pytest.raises(G.GbwtHipError) as e:
            call()
        assert e.value.status == _lib.BAD_ARGUMENT and len(str(e.value)) > len("BAD_ARGUMENT: ")
    for call in (lambda: dev.links_csr([0], [0]), dev.graph_lines):
        with pytest.raises(G.GbwtHipError) as e:
            call()
        assert NEEDS_GFA in str(e.value)


# ---- shapes that break a decoder or the canonical rule -------------------------------------------------------------------------------------------

def self_loops():
    """Every kind of self-loop and hairpin, on nodes of a path and on nodes of their own, and two nodes joined in all four ways."""
    fwd, rev = TG.fwd, TG.rev
    paths = [[fwd(v) for v in range(1, 40)]]
    for k, x in enumerate(list(range(3, 36, 3)) + list(range(40, 60))):
        paths.append(([fwd(x), fwd(x)], [rev(x), rev(x)], [fwd(x), rev(x)], [rev(x), fwd(x)], [fwd(x), fwd(x), rev(x), rev(x), fwd(x)])[k % 5])
    paths += [[fwd(70), fwd(71)], [fwd(70), rev(71)], [rev(70), fwd(71)], [rev(70), rev(71)], [fwd(71), fwd(70)]]
    return [np.array(p, dtype=np.uint64) for p in paths], True


def fans():
    """Hubs with 1, 2, 63, 64, 65, 66, 1023, 1024, 1025, 1026 and 2049 edges, forward and reverse: rows at the hand-off from a lane to a
    workgroup (64 edges; a leading ENDMARKER edge does not count) and at the stretches the workgroup stages (1 024 nodes)."""
    paths, leaf = [], 100
    for hub, degree in enumerate((1, 2, 63, 64, 65, 66, 1023, 1024, 1025, 1026, 2049), start=1):
        for k in range(degree):
            paths.append([TG.fwd(hub), TG.fwd(leaf + k) if k % 3 else TG.rev(leaf + k)])
        if hub % 2 == 0:
            paths.append([TG.fwd(hub)])                        # (the hub's record also ends a path: an ENDMARKER edge in front)
        leaf += degree
    return [np.array(p, dtype=np.uint64) for p in paths], True


SHAPES = {
    "tree-with-hub": TG.tree_with_hub,
    "reverse-joins": TG.reverse_joins,
    "interleaved": TG.interleaved,
    "self-loops": self_loops,
    "fans": fans,
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_edges_and_graph_text(tmp_path, name):
    paths, _ = SHAPES[name]()
    path = str(tmp_path / "graph.gbz")
    S.Synth.from_paths(paths).attach_gbz(seed=3).save(path, as_gbz=True)
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    graph = X.Graph(oracle.gbwt())
    assert dev.node_iter().tolist() == graph.node_ids()
    ids, orient = both_orientations(np.arange(0, graph.max_node + 3))
    check_edges(dev, graph, ids, orient)
    check_edges(dev, graph, *mixed_request(graph, 31))
    if name == "tree-with-hub":
        assert max(len(r) for r in graph.rows.values()) >= 5000
    want = check_graph_text(dev, oracle, tmp_path)
    if name in ("tree-with-hub", "reverse-joins", "interleaved"):
        assert graph.max_node >= 99999 and len(want) > 300 * 4096        # ids of one to six digits; hundreds of workgroups of text
    if name in ("self-loops", "reverse-joins"):
        fields = [l.split(b"\t") for l in X.lines_of(want, b"L").splitlines()]
        assert {f[2] for f in fields if f[1] == f[3]} == {b"+", b"-"}      # loops from both orientations are among the L-lines


def test_unidirectional_bare_handle_has_no_reverse_records():
    paths, bidirectional = TG.permuted_path_unidirectional()
    s = S.Synth.from_paths(paths, bidirectional=bidirectional)
    dev = G.GBWT.from_records(s.data(), s.starts(), s.alphabet_offset, s.alphabet_size, s.sequences, s.size, bidirectional)
    oracle = O.OracleGBWT.from_bwt(O.OracleBWT.from_parts(s.data(), s.starts()), s.sequences, s.size, s.alphabet_offset, s.alphabet_size, bidirectional)
    graph = X.Graph(oracle)
    ids, orient = both_orientations(np.arange(0, graph.max_node + 3))
    rows = [graph.edges(int(i), int(o)) for i, o in zip(ids, orient)]
    assert sum(r is not None for r in rows[0::2]) >= 99999 and all(r is None for r in rows[1::2])
    check_edges(dev, graph, ids, orient)
    check_edges(dev, graph, *mixed_request(graph, 32))
    assert dev.node_iter().tolist() == graph.node_ids()


# ---- long labels --------------------------------------------------------------------------------------------------------------------------

def test_long_labels_tangle(tmp_path):
    lengths = TG.tangle_label_lengths()
    paths, _ = TG.tangle(lengths=lengths)
    path = str(tmp_path / "tangle.gbz")
    S.Synth.from_paths(paths).attach_gbz(seed=3, label_lengths=lengths).save(path, as_gbz=True)
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    want = check_graph_text(dev, oracle, tmp_path)
    sizes = [len(l.split(b"\t")[2]) for l in X.lines_of(want, b"S").splitlines()]
    assert min(sizes) == 1 and max(sizes) == TG.TANGLE_GIANT


def test_long_labels_largest(tmp_path):
    lengths, paths = TG.long_label(LARGEST_LABEL)
    path = str(tmp_path / "largest.gbz")
    S.Synth.from_paths(paths).attach_gbz(seed=5, label_lengths=lengths).save(path, as_gbz=True)
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    want = X.graph_text(oracle.gfa())
    got = dev.graph_lines()
    assert len(got) == len(want) > LARGEST_LABEL and got == want


# ---- a synthetic translation --------------------------------------------------------------------------------------------------------------

def translated(tmp_path, tag=None):
    """Segments of 1, 2 and many nodes, one whose nodes are on no path (segment_iter skips it, its links are None), a hub segment with 1 500
    links, hairpins and reverse joins between segments.  (Every node of a path gets a record and the generator's translation covers every node
    id: a successor without a segment cannot be generated; tests/test_graph_expect_cpu.py pins that rule by hand.)"""
    fwd, rev = TG.fwd, TG.rev
    rng = np.random.default_rng(41)
    starts = [1, 2, 4, 9, 10, 13, 15, 16, 40]                    # [1] [2,3] [4..8] [9] [10..12]: unused [13,14] [15] [16..39] [40 ...] then singles
    starts += list(range(41, 41 + 1500)) + list(range(1541, 1599, 2))
    walk = lambda a, b: [fwd(v) for v in range(a, b + 1)]
    back = lambda a, b: [rev(v) for v in range(b, a - 1, -1)]
    paths = [walk(1, 9) + walk(13, 40), back(4, 8) + walk(2, 3) + back(16, 39) + walk(15, 15), walk(4, 8) + walk(4, 8), walk(2, 3) + back(2, 3), back(13, 14) + walk(13, 14),
             walk(16, 39) + back(1, 1), walk(9, 9) + walk(9, 9), back(9, 9) + walk(15, 15) + back(15, 15)]
    for k in range(1500):                                      # the hub: segment [16..39] forward to 1 500 single-node segments
        paths.append(walk(16, 39) + ([fwd(41 + k)] if k % 4 else [rev(41 + k)]))
    for v in range(1541, 1599, 2):                             # two-node segments: a hairpin, a loop, or on to a random single-node segment
        single = int(rng.integers(41, 1541))
        paths.append(walk(v, v + 1) + (back(v, v + 1), walk(v, v + 1), [rev(single)], [fwd(single)])[(v // 2) % 4])
    s = S.Synth.from_paths([np.array(p, dtype=np.uint64) for p in paths]).attach_gbz(starts, seed=7)
    if tag:
        s.set_tag("reference_samples", tag)
    path = str(tmp_path / ("tagged.gbz" if tag else "translated.gbz"))
    s.save(path, as_gbz=True)
    return path, starts


def test_synthetic_translation_links_segments_and_text(tmp_path):
    path, starts = translated(tmp_path)
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    graph = X.Graph(oracle.gbwt())
    gfa = oracle.gfa()
    t = X.Translation.from_starts(graph, starts, X.segment_names(gfa), graph.max_node + 1)
    assert 4 not in t.segment_ids() and t.links(4, 0) is None and len(t.links(7, 0)) > 1500
    assert sorted({b - a for _, _, a, b in t.segments}) == [1, 2, 3, 5, 24]
    seg_ids, seg_orient = both_orientations(np.arange(0, len(t.segments) + 2))
    check_links(dev, t, seg_ids, seg_orient)
    rng = np.random.default_rng(42)
    pick = rng.integers(0, len(t.segments) + 3, size=4000).astype(np.uint64)
    pick[:3] = [1 << 40, (1 << 64) - 1, 4]
    check_links(dev, t, pick, rng.integers(0, 2, size=pick.size).astype(np.uint8))
    assert dev.segment_iter().tolist() == t.segment_ids()
    nodes = np.arange(0, graph.max_node + 3, dtype=np.uint64)
    got, valid = dev.node_to_segments(nodes)
    want = [t.node_to_segment(int(v)) for v in nodes]
    assert valid.tolist() == [w is not None for w in want] and got[valid].tolist() == [w for w in want if w is not None]
    ids, orient = both_orientations(nodes)
    check_edges(dev, graph, ids, orient)
    check_graph_text(dev, oracle, tmp_path)
    assert X.link_lines(graph, t) == X.lines_of(gfa, b"L")


def test_reference_samples_header(tmp_path):
    path, _ = translated(tmp_path, tag="s0 s3")
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    want = check_graph_text(dev, oracle, tmp_path)
    assert want.startswith(b"H\tVN:Z:1.1\tRS:Z:s0 s3\n")


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------

def test_plumbing_empty_capacity_workspaces_device_forms_and_times():
    import torch
    from gbwt_rs_amd import dist
    path = os.path.join(O.GOLDEN, "translation.gbz")
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    graph = X.Graph(oracle.gbwt())
    L = _lib.lib()
    # before any request
    with pytest.raises(G.GbwtHipError) as e:
        dev.last_graph_ms()
    assert e.value.status == _lib.BAD_ARGUMENT
    # n = 0
    for got in (dev.edges_csr([], []), dev.edges_csr([], [], True), dev.links_csr([], [])):
        assert got[0].tolist() == [0] and got[1].size == 0 and got[2].size == 0
    rows = dev.edges_device([], [])
    assert (rows.n, rows.total) == (0, 0)
    # the size query, then a capacity that is too small
    ids, orient = both_orientations(np.arange(0, graph.max_node + 3))
    for fn in (L.gbwt_hip_edges, L.gbwt_hip_links):
        offsets, valid, total = np.zeros(ids.size + 1, dtype=np.uint64), np.zeros(ids.size, dtype=np.uint8), C.c_uint64(0)
        assert fn(dev._h, dev._ws, ids.ctypes.data, orient.ctypes.data, ids.size, 0, offsets.ctypes.data, None, 0, C.byref(total), valid.ctypes.data) == _lib.OK
        assert total.value == int(offsets[-1]) > 1
        out = np.zeros(total.value, dtype=np.uint64)
        assert fn(dev._h, dev._ws, ids.ctypes.data, orient.ctypes.data, ids.size, 0, offsets.ctypes.data, out.ctypes.data, total.value - 1, C.byref(total),
                  valid.ctypes.data) == _lib.CAPACITY
        assert fn(dev._h, dev._ws, ids.ctypes.data, orient.ctypes.data, ids.size, 0, offsets.ctypes.data, out.ctypes.data, total.value, C.byref(total), valid.ctypes.data) == _lib.OK
    total = C.c_uint64(0)
    assert L.gbwt_hip_graph_lines(dev._h, dev._ws, None, 0, C.byref(total)) == _lib.OK and total.value == len(X.graph_text(oracle.gfa()))
    buf = C.create_string_buffer(total.value)
    assert L.gbwt_hip_graph_lines(dev._h, dev._ws, buf, total.value - 1, C.byref(total)) == _lib.CAPACITY
    count = C.c_uint64(0)
    assert L.gbwt_hip_node_ids(dev._h, None, 0, C.byref(count)) == _lib.OK and count.value == len(graph.node_ids())
    few = np.zeros(count.value, dtype=np.uint64)
    assert L.gbwt_hip_node_ids(dev._h, few.ctypes.data, count.value - 1, C.byref(count)) == _lib.CAPACITY
    assert L.gbwt_hip_segments(dev._h, few.ctypes.data, 1, C.byref(count)) == _lib.CAPACITY and count.value == 7
    # a second call and a second workspace answer the same
    other = dev.another_workspace()
    first = dev.edges_csr(ids, orient, True)
    for again in (dev.edges_csr(ids, orient, True), other.edges_csr(ids, orient, True)):
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    seg_ids, seg_orient = both_orientations(np.arange(0, 10))
    first = dev.links_csr(seg_ids, seg_orient)
    for again in (dev.links_csr(seg_ids, seg_orient), other.links_csr(seg_ids, seg_orient)):
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    text = dev.graph_lines()
    assert text == X.graph_text(oracle.gfa()) and dev.graph_lines() == text and other.graph_lines() == text
    # the device forms, copied back with torch
    for predecessors in (False, True):
        got = dev.rows_to_host(dev.edges_device(ids, orient, predecessors))
        assert all(np.array_equal(a, b) for a, b in zip(got, dev.edges_csr(ids, orient, predecessors)))
        got = dev.rows_to_host(dev.links_device(seg_ids, seg_orient, predecessors))
        assert all(np.array_equal(a, b) for a, b in zip(got, dev.links_csr(seg_ids, seg_orient, predecessors)))
    for _ in range(2):                                         # the second request formats from the kept sizes
        view = dev.graph_lines_device()
        size = view.header_bytes + view.segment_bytes + view.link_bytes
        assert bytes(dist.device_view(view.d_text, size, torch.uint8, torch.device("cuda", 0)).cpu().numpy()) == text
    sizes_ms, segments_ms, links_ms = dev.last_graph_ms()
    assert sizes_ms == 0 and segments_ms > 0 and links_ms > 0
    fresh = dev.another_workspace()
    fresh.graph_lines_device()
    assert fresh.last_graph_ms()[0] > 0
