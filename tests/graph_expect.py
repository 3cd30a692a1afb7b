"""What the graph API must answer, in plain Python over the oracle: the edges of a node from OracleRecord.edges(), links through a
node-to-segment table, the graph text as the H-, S- and L-lines of OracleGBZ.gfa().  Shared by tests/test_graph_expect_cpu.py (which pins it
to the reference's documented answers and to the oracle's L-lines) and tests/test_gpu_graph_api.py.

The rules restated here (file:line into the reference):
  has_node(id)                    the forward record of the node holds an edge                       src/gbz.rs:286-289
  successors / predecessors       EdgeIter over the record of (id, o) / of (id, flip o), flipped     src/gbz.rs:327-353, 819-870
  segment_successors / _pred.     the edges of the boundary node, mapped; ends at a node without a segment   src/gbz.rs:402-440, 988-1005
  canonical links                 forward: to >= from; reverse: to > from, or to == from forward     src/bin/gbunzip.rs:271-317"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def known():
    """The reference's documented answers (tests/golden/graph_known.json: names and numbers only)."""
    with open(os.path.join(GOLDEN, "graph_known.json")) as f:
        return json.load(f)


class Graph:
    """The nodes and edges of an index, from the oracle's records (any OracleGBWT, bidirectional or not)."""

    def __init__(self, gbwt):
        self.offset, self.size = gbwt.alphabet_offset(), gbwt.alphabet_size()
        bwt = gbwt.bwt()
        self.rows = {}                                       # GBWT node -> [successor GBWT nodes], for the records that exist
        for node in range(self.offset + 1, self.size):
            rec = bwt.record(node - self.offset)
            if rec is not None:
                self.rows[node] = [int(succ) for succ, _ in rec.edges()]
        self.min_node, self.max_node = (self.offset + 1) // 2, self.size // 2 - 1 if self.size else 0

    def has_node(self, node_id):
        return 2 * node_id in self.rows

    def node_ids(self):
        return [v // 2 for v in sorted(self.rows) if v % 2 == 0]

    def edges(self, node_id, orientation, predecessors=False):
        """[(id, orientation), ...] or None, as GBZ::successors / predecessors."""
        if node_id <= 0 or not self.has_node(node_id):
            return None
        flip = 1 if predecessors else 0
        row = self.rows.get(2 * node_id + (orientation ^ flip))
        if row is None:
            return None
        if row and row[0] == 0:                              # the ENDMARKER edge (EdgeIter::new)
            row = row[1:]
        return [(v // 2, (v & 1) ^ flip) for v in row]


class Translation:
    """Segments as (id, name, first node, one past the last node); node_to_segment through a table."""

    def __init__(self, graph, segments):
        self.graph = graph
        self.segments = [(int(i), name, int(a), int(b)) for i, name, a, b in segments]
        self.of = {}
        for i, _, a, b in self.segments:
            for v in range(a, b):
                self.of[v] = i

    @classmethod
    def from_starts(cls, graph, segment_starts, names, mapping_len):
        """segment_starts of the generator (attach_gbz) and the names -- for the segments whose first node exists, those of the oracle's
        S-lines, in order; the others are never printed and get their generated name."""
        starts = [int(x) for x in segment_starts]
        ends = starts[1:] + [int(mapping_len)]
        listed = iter(names)
        segments = []
        for i, (a, b) in enumerate(zip(starts, ends)):
            segments.append((i, next(listed) if graph.has_node(a) else f"seg{a}", a, b))
        assert next(listed, None) is None
        return cls(graph, segments)

    def node_to_segment(self, node_id):
        return self.of.get(node_id) if self.graph.has_node(node_id) else None

    def segment_ids(self):
        return [i for i, _, a, _ in self.segments if self.graph.has_node(a)]

    def links(self, segment_id, orientation, predecessors=False):
        """[(segment id, orientation), ...] or None, as GBZ::segment_successors / segment_predecessors."""
        if not 0 <= segment_id < len(self.segments):
            return None
        _, _, a, b = self.segments[segment_id]
        if a >= b:
            return None
        node = b - 1 if (orientation == 0) != bool(predecessors) else a
        return map_links(self.graph.edges(node, orientation, predecessors), self.node_to_segment)


def map_links(edges, node_to_segment):
    """LinkIter over an edge row: every node replaced by its segment; the row ends in front of the first node without one."""
    if edges is None:
        return None
    out = []
    for node_id, o in edges:
        seg = node_to_segment(node_id)
        if seg is None:
            break
        out.append((seg, o))
    return out


def canonical(from_id, from_rev, to_id, to_rev):
    return (to_id > from_id or (to_id == from_id and not to_rev)) if from_rev else to_id >= from_id


def link_lines(graph, translation=None):
    """The L-lines gbunzip writes, rebuilt from the edge rows with the canonical rule."""
    sign = "+-"
    out = []
    if translation is None:
        for v in graph.node_ids():
            for o in (0, 1):
                for to, to_o in graph.edges(v, o) or []:
                    if canonical(v, o, to, to_o):
                        out.append(f"L\t{v}\t{sign[o]}\t{to}\t{sign[to_o]}\t*\n")
    else:
        name = {i: n for i, n, _, _ in translation.segments}
        for s in translation.segment_ids():
            for o in (0, 1):
                for to, to_o in translation.links(s, o) or []:
                    if canonical(s, o, to, to_o):
                        out.append(f"L\t{name[s]}\t{sign[o]}\t{name[to]}\t{sign[to_o]}\t*\n")
    return "".join(out).encode()


def graph_text(gfa):
    """The lines of a GFA file that start with H, S or L (they precede the paths and walks)."""
    return b"".join(line for line in gfa.splitlines(keepends=True) if line[:1] in (b"H", b"S", b"L"))


def lines_of(gfa, kind):
    return b"".join(line for line in gfa.splitlines(keepends=True) if line[:1] == kind)


def segment_names(gfa):
    return [line.split(b"\t")[1].decode() for line in gfa.splitlines() if line[:1] == b"S"]


def csr(rows):
    """(offsets uint64[n + 1], flat uint64, valid bool[n]) of a list of rows ([(id, orientation), ...] or None)."""
    offsets = np.zeros(len(rows) + 1, dtype=np.uint64)
    np.cumsum([0 if r is None else len(r) for r in rows], out=offsets[1:])
    flat = np.array([2 * i + o for r in rows if r for i, o in r], dtype=np.uint64)
    return offsets, flat, np.array([r is not None for r in rows], dtype=bool)
