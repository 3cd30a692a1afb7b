"""The truth of the locate queries (include/gbwt_hip.h, "locate"), stated without the library: the oracle's own start / forward walk of every
sequence tells which sequence owns every BWT position.  The reference has no locate of its own to be compared with.  Pinned on the CPU in
tests/test_locate_cpu.py."""
import numpy as np


class Owners(dict):
    """{(node, offset): sequence id}, with the record lengths of its index (`lengths`) for the validity rules."""


def owners(gbwt):
    """{(node, offset): sequence id} over every visit of every sequence of an OracleGBWT."""
    out = Owners()
    out.lengths = Lengths(gbwt)
    for seq in range(gbwt.sequences()):
        pos = gbwt.start(seq)
        while pos is not None:
            assert pos not in out, f"position {pos} is a visit of sequences {out[pos]} and {seq}"
            out[pos] = seq
            pos = gbwt.forward(pos)
    return out


class Lengths:
    """Record::len of the record of a node, None where GBWT::find finds no record: the endmarker, a node at or below the alphabet offset, at or
    past the alphabet size, a node without a record."""

    def __init__(self, gbwt):
        self.gbwt, self.bwt, self.memo = gbwt, gbwt.bwt(), {}

    def of(self, node):
        node = int(node)
        if node not in self.memo:
            g, value = self.gbwt, None
            if g.alphabet_offset() < node < g.alphabet_size():
                rec = self.bwt.record(node - g.alphabet_offset())
                value = None if rec is None else rec.len()
            self.memo[node] = value
        return self.memo[node]


def row(own, state, unique):
    """The ids of state (node, start, end), or None for an invalid state."""
    node, start, end = (int(x) for x in state)
    n = own.lengths.of(node)
    if n is None or start >= end or end > n:
        return None
    ids = [own[(node, i)] for i in range(start, end)]
    return sorted(set(ids)) if unique else ids


def position(own, pos):
    """The id of position (node, offset), or None."""
    node, offset = int(pos[0]), int(pos[1])
    n = own.lengths.of(node)
    return None if n is None or offset >= n else own[(node, offset)]


def csr(rows):
    """(offsets, ids, valid) of a list of rows (None = invalid), as the library returns them."""
    offsets = np.zeros(len(rows) + 1, dtype=np.uint64)
    np.cumsum([0 if r is None else len(r) for r in rows], out=offsets[1:])
    flat = np.array([x for r in rows if r is not None for x in r], dtype=np.uint64)
    return offsets, flat, np.array([r is not None for r in rows], dtype=bool)
