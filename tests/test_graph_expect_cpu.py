"""tests/graph_expect.py pinned on the CPU: to the answers the reference documents (tests/golden/graph_known.json) and to the L-lines of the
oracle's GFA, rebuilt from its edge rows with the canonical rule.  No GPU."""
import os

import numpy as np

import graph_expect as X
import oracle_lib as O
from gbwt_rs_amd import synth as S

KNOWN = X.known()


def golden(name):
    oracle = O.OracleGBZ(os.path.join(O.GOLDEN, name))
    return oracle, X.Graph(oracle.gbwt())


def translation_of(graph):
    return X.Translation(graph, [(i, name, a, b) for i, name, a, b, _ in KNOWN["translation.gbz"]["segments"]])


def test_documented_edges_of_the_example():
    _, graph = golden("example.gbz")
    for key, predecessors in (("successors", False), ("predecessors", True)):
        for case in KNOWN["example.gbz"][key]:
            assert graph.edges(case["node"], case["orientation"], predecessors) == [tuple(e) for e in case["edges"]]
    assert graph.has_node(24) and graph.has_node(14) and not graph.has_node(0) and not graph.has_node(graph.max_node + 1)
    assert graph.edges(0, 0) is None and graph.edges(graph.max_node + 1, 1, True) is None
    assert graph.node_ids() == sorted(graph.node_ids()) and graph.min_node <= graph.node_ids()[0] and graph.node_ids()[-1] <= graph.max_node


def test_documented_segments_and_links_of_the_translation():
    oracle, graph = golden("translation.gbz")
    t = translation_of(graph)
    rows = KNOWN["translation.gbz"]["segments"]
    by_name = {name: i for i, name, _, _, _ in rows if name}
    assert rows[0] == [0, "s11", 1, 3, "GAT"]
    first = t.segment_ids()[0]
    assert t.segments[first] == (0, "s11", 1, 3)
    # the S-lines of the oracle carry exactly the segments whose first node exists, with the documented names and sequences
    s_lines = X.lines_of(oracle.gfa(), b"S").decode().splitlines()
    assert s_lines == [f"S\t{rows[i][1]}\t{rows[i][4]}" for i in t.segment_ids()]
    assert 4 not in t.segment_ids() and t.links(4, 0) is None and t.links(len(rows), 0) is None
    for key, predecessors in (("segment_successors", False), ("segment_predecessors", True)):
        for case in KNOWN["translation.gbz"][key]:
            want = [(by_name[name], o) for name, o in case["links"]]
            assert t.links(by_name[case["segment"]], case["orientation"], predecessors) == want
    assert t.node_to_segment(5) == by_name["s14"] and t.node_to_segment(6) == by_name["s14"] and t.node_to_segment(7) is None


def test_a_link_row_ends_at_the_first_node_without_a_segment():
    """LinkIter::next returns None there (src/gbz.rs:996-999).  The generator cannot make such a graph -- every node of a path gets a record
    and its translation covers every node id -- so the rule is pinned on an edge row written by hand."""
    table = {1: 0, 2: 0, 3: 1, 5: 2}
    assert X.map_links([(3, 0), (5, 1), (4, 0), (1, 1)], table.get) == [(1, 0), (2, 1)]
    assert X.map_links([(4, 1), (3, 0)], table.get) == []
    assert X.map_links(None, table.get) is None and X.map_links([], table.get) == []


def test_canonical_rule_on_self_loops():
    assert X.canonical(5, 0, 5, 0) and X.canonical(5, 0, 5, 1) and X.canonical(5, 1, 5, 0) and not X.canonical(5, 1, 5, 1)
    assert X.canonical(5, 0, 6, 1) and not X.canonical(5, 0, 4, 0) and X.canonical(5, 1, 6, 1) and not X.canonical(5, 1, 4, 0)


def test_rebuilt_link_lines_equal_the_oracle_on_the_golden_files():
    oracle, graph = golden("example.gbz")
    assert X.link_lines(graph) == X.lines_of(oracle.gfa(), b"L")
    oracle, graph = golden("translation.gbz")
    assert X.link_lines(graph, translation_of(graph)) == X.lines_of(oracle.gfa(), b"L")
    text = X.graph_text(oracle.gfa())
    assert text.startswith(b"H\tVN:Z:1.1") and oracle.gfa().startswith(text)


def test_rebuilt_link_lines_equal_the_oracle_on_a_synthetic(tmp_path):
    """Hairpins, self-loops in both orientations and a translation with segments of 1, 2 and 4 nodes, one of them without nodes."""
    fwd, rev = (lambda v: 2 * v), (lambda v: 2 * v + 1)
    paths = [[fwd(1), fwd(2), fwd(3), rev(4), fwd(5), fwd(6), fwd(7), fwd(8), fwd(11)], [fwd(3), fwd(3)], [rev(4), rev(4)], [fwd(5), rev(5)], [rev(11), fwd(11), fwd(1)],
             [rev(8), rev(7), rev(6), rev(5), fwd(4), rev(2), rev(1)]]
    starts = [1, 3, 4, 5, 9, 11]                                 # [1,2] [3] [4] [5..8] [9,10]: no nodes [11]
    plain, translated = str(tmp_path / "plain.gbz"), str(tmp_path / "translated.gbz")
    S.Synth.from_paths(paths).attach_gbz(seed=2).save(plain, as_gbz=True)
    S.Synth.from_paths(paths).attach_gbz(starts, seed=2).save(translated, as_gbz=True)
    oracle = O.OracleGBZ(plain)
    graph = X.Graph(oracle.gbwt())
    assert graph.node_ids() == [1, 2, 3, 4, 5, 6, 7, 8, 11]
    assert X.link_lines(graph) == X.lines_of(oracle.gfa(), b"L")
    oracle = O.OracleGBZ(translated)
    gfa = oracle.gfa()
    t = X.Translation.from_starts(graph, starts, X.segment_names(gfa), 12)
    assert t.segment_ids() == [0, 1, 2, 3, 5] and t.links(4, 0) is None and t.links(4, 1, True) is None
    assert X.link_lines(graph, t) == X.lines_of(gfa, b"L")
    offsets, flat, valid = X.csr([t.links(s, o) for s in range(7) for o in (0, 1)])
    assert offsets.dtype == np.uint64 and int(offsets[-1]) == flat.size and valid.tolist() == [True] * 8 + [False] * 2 + [True] * 2 + [False] * 2
