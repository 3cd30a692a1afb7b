"""The graphs of the suite moved up the node id range: every node id plus d, so that the smallest id is far from 1 and the largest reaches
2^31 - 1, the library's stated limit (alphabet_size 2^32, every GBWT node word with bit 31 set, ten-digit ids in the text).  A shift changes
nothing but the ids: the oracle's answers over a shifted file are its answers over the unshifted one, moved (tests/test_shifted_cpu.py pins
that on the CPU), so the expectations of a shifted graph are the existing helpers' expectations over the UNSHIFTED oracle file, moved by the
functions below -- the id-indexed helpers (seq_expect.LabelTable, tags_expect.tag_text, tangled_graphs.Expected) are never asked for
tables of 2^31 entries.  Plain Python and numpy: shared by the CPU and the GPU tests."""
import copy

import numpy as np

MAX_NODE_ID = (1 << 31) - 1                       # the library's limit: node ids 1 .. 2^31 - 1


def SHIFTS(max_id):
    """The three shifts by name, for a path set whose largest node id is max_id."""
    max_id = int(max_id)
    return {
        "million": 1000003,                       # seven-digit ids; id-indexed tables of the helpers still fit
        "straddle": (1 << 30) - max_id // 2,      # the GBWT nodes 2 * id + o lie on both sides of 2^31
        "top": MAX_NODE_ID - max_id,              # the largest id is 2^31 - 1, alphabet_size is 2^32
    }


SHIFT_NAMES = ("million", "straddle", "top")


def max_id_of(paths):
    return max((int(np.asarray(p, dtype=np.uint64).max()) >> 1 for p in paths if len(p)), default=0)


def shift_paths(paths, d):
    """Every GBWT-encoded node (2 * id + orientation) plus 2 * d; empty paths stay empty."""
    return [np.asarray(p, dtype=np.uint64) + np.uint64(2 * d) for p in paths]


def _name(field, d):
    return b"%d" % (int(field) + d)


def shift_gfa(text, d):
    """A GFA text with d added to the segment name of S-lines, both names of L-lines, every step of P-lines and every > / < step of W-lines.
    Everything else -- labels, the start and end coordinates of W-lines, H-lines, overlap fields, a missing last newline -- stays."""
    out = []
    for line in text.split(b"\n"):
        f = line.split(b"\t")
        kind = f[0]
        if kind == b"S":
            f[1] = _name(f[1], d)
        elif kind == b"L":
            f[1], f[3] = _name(f[1], d), _name(f[3], d)
        elif kind == b"P":
            f[2] = b",".join(_name(s[:-1], d) + s[-1:] for s in f[2].split(b",")) if f[2] else f[2]
        elif kind == b"W":
            walk = f[6].replace(b">", b" >").replace(b"<", b" <").split()
            f[6] = b"".join(s[:1] + _name(s[1:], d) for s in walk)
        out.append(b"\t".join(f))
    return b"\n".join(out)


# ---- moving an expectation ----------------------------------------------------------------------------------------------------------------

def move_nodes(nodes, d):
    """GBWT-encoded nodes (node rows, edge rows) plus 2 * d, as uint64."""
    return np.asarray(nodes).astype(np.uint64) + np.uint64(2 * d)


def move_tags(tags, d):
    """Tags ((id << 11) | (orientation << 10)) + offset plus d << 11; the 0 of an endmarker stays."""
    tags = np.asarray(tags, dtype=np.uint64)
    return np.where(tags != 0, tags + np.uint64(d << 11), np.uint64(0))


def move_ids(ids, d):
    """Node ids plus d, as uint64."""
    return np.asarray(ids).astype(np.uint64) + np.uint64(d)


def move_expected(want, d):
    """A tangled_graphs.Expected (built over the unshifted paths) with min_node and the node ids plus d; the rest does not change."""
    moved = copy.copy(want)
    if want.slots:
        moved.min_node = want.min_node + d
        moved.ids = move_ids(want.ids, d)
    return moved


def move_positions(positions, d):
    """uint64[m, 2] GBWT positions (node, offset) with the node plus 2 * d."""
    moved = np.array(positions, dtype=np.uint64).reshape(-1, 2)
    moved[:, 0] += np.uint64(2 * d)
    return moved
