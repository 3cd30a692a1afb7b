"""Graphs for the FM-index family of paths (GBZ.suffix_array, GBZ.fm_index, seeds, chains), written as GFA text -- S-, L- and W-lines, W-lines
only, so that path ids are the file order -- in which every label and every walk is chosen here, and the yardstick of their texts derived
from the same Python data and never from the device: the bases of a path (labels joined along the walk, a `<` step reverse-complemented),
the text and the bounds (the cumulated len + 1) of a list of path ids in any order, and the tag of every text position through
tags_expect.gfa_rows and tags_expect.tag_text.  Plain Python and numpy, without the library: shared by the CPU and the GPU tests.

tangle_small(): 40 nodes with labels of 1, 2, 15, 16, 17, 31, 33 and one of 200 bases (16 is the anchor stride of the seeds), eight walks of
1, 2, 3 and a few dozen steps with reversed steps, immediate repeats `x x` and `x rev(x)`, revisits, the 200-base node in both orientations,
two equal walks and one that is the reverse of another.
periodic(reps): one node AC; path k visits it reps[k] times."""
import numpy as np

import fm_expect as F
import seed_expect as E
import tags_expect as T

_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")

FORWARD, REVERSE = 0, 1


def reverse_complement(bases):
    return bytes(bases).translate(_COMPLEMENT)[::-1]


class PathGraph:
    """labels: {node id: bytes}; walks: one list of (node id, orientation) per path, path id = place in the list."""

    def __init__(self, labels, walks):
        self.labels = {int(k): bytes(v) for k, v in labels.items()}
        self.walks = [[(int(v), int(o)) for v, o in walk] for walk in walks]
        assert all(v in self.labels for walk in self.walks for v, _ in walk) and all(self.walks)

    def paths(self):
        return len(self.walks)

    def gfa(self):
        """The GFA text: H, the S-lines by id, one L-line for every pair of steps that follow each other on a walk, the W-lines in path order
        (sample s, haplotype = path id + 1, contig c: the four fields of two equal walks still differ)."""
        lines = [b"H\tVN:Z:1.1"]
        lines += [b"S\t%d\t%s" % (v, self.labels[v]) for v in sorted(self.labels)]
        links = sorted({(a, b) for walk in self.walks for a, b in zip(walk[:-1], walk[1:])})
        lines += [b"L\t%d\t%s\t%d\t%s\t0M" % (a[0], b"+-"[a[1]:a[1] + 1], b[0], b"+-"[b[1]:b[1] + 1]) for a, b in links]
        for p, walk in enumerate(self.walks):
            steps = b"".join(b"<>"[1 - o:2 - o] + b"%d" % v for v, o in walk)
            lines.append(b"W\ts\t%d\tc\t0\t%d\t%s" % (p + 1, len(self.row_text(p)), steps))
        return b"\n".join(lines) + b"\n"

    def step_text(self, step):
        v, o = step
        return reverse_complement(self.labels[v]) if o else self.labels[v]

    def row_text(self, p):
        """The bases of path p."""
        return b"".join(self.step_text(step) for step in self.walks[p])

    def step_starts(self, p):
        """The offset in row_text(p) of the first base of every step of path p."""
        at, out = 0, []
        for v, _ in self.walks[p]:
            out.append(at)
            at += len(self.labels[v])
        return out

    def text(self, order, endmarker=0):
        """The text of the paths `order`: the bases of each with the endmarker byte behind it."""
        return b"".join(self.row_text(p) + bytes([endmarker]) for p in order)

    def bounds(self, order):
        """The text offset of every path of `order` and the length of the text: the cumulated len + 1."""
        out = [0]
        for p in order:
            out.append(out[-1] + len(self.row_text(p)) + 1)
        return out

    def tags(self, order):
        """The tag of every position of text(order, .): ((id << 11) | (orientation << 10)) + offset inside the node, 0 on an endmarker.  The
        rows are read back from the W-lines of the GFA text, the label lengths from this object."""
        rows = T.gfa_rows(self.gfa())
        assert len(rows) == len(self.walks)
        lengths = np.zeros(max(self.labels) + 1, dtype=np.int64)
        for v, label in self.labels.items():
            lengths[v] = len(label)
        tags, offsets = T.tag_text(lengths, [rows[p] for p in order])
        assert offsets.tolist() == self.bounds(order)
        return tags

    def visits(self, order, node, orientation):
        """[(place k in `order`, step)] of every visit of `node` in this orientation."""
        return [(k, s) for k, p in enumerate(order) for s, step in enumerate(self.walks[p]) if step == (node, orientation)]


def from_gfa(gfa):
    """The PathGraph of a GFA text whose segment names are node ids: labels from the S-lines, walks from the P- and W-lines in file order."""
    labels = {int(f[1]): f[2] for f in (line.split(b"\t") for line in gfa.split(b"\n")) if f[0] == b"S"}
    return PathGraph(labels, [[(int(v) >> 1, int(v) & 1) for v in row] for row in T.gfa_rows(gfa)])


LABEL_LENGTHS = (1, 2, 15, 16, 17, 31, 33)
LONG_NODE, LONG_LENGTH = 40, 200
ONE_STEP_PATH = 1                                  # path 1 of tangle_small: one visit of node 1, whose label is one base


def reversed_walk(walk):
    return [(v, 1 - o) for v, o in walk[::-1]]


def random_walk(rng, steps, nodes):
    """`steps` visits of these nodes, about 30 % of them reversed."""
    return [(int(nodes[int(rng.integers(0, len(nodes)))]), int(rng.random() < 0.3)) for _ in range(steps)]


def tangle_small(seed=7):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
    labels = {v: alphabet[rng.integers(0, 4, size=LABEL_LENGTHS[(v - 1) % len(LABEL_LENGTHS)])].tobytes() for v in range(1, LONG_NODE)}
    labels[LONG_NODE] = alphabet[rng.integers(0, 4, size=LONG_LENGTH)].tobytes()
    short = list(range(1, LONG_NODE))
    # A: a dozen steps with an immediate repeat x x and a node read forward and at once in reverse
    a = random_walk(rng, 4, short) + [(9, 0), (9, 0)] + random_walk(rng, 3, short) + [(17, 0), (17, 1)] + random_walk(rng, 2, short)
    # B: two dozen steps, the long node forward, a reverse repeat and nodes of A revisited; its reverse is a path too
    b = random_walk(rng, 7, short) + [(LONG_NODE, 0)] + random_walk(rng, 5, short) + [(24, 1), (24, 1)] + a[1:4] + random_walk(rng, 6, short) + [(3, 1), (3, 0)]
    # C: three dozen steps that go through the nodes of A and B again and through every node not yet seen
    seen = {v for v, _ in a + b}
    rest = [(v, int(rng.random() < 0.3)) for v in short if v not in seen]
    c = random_walk(rng, 5, short) + rest[: len(rest) // 2] + b[2:6] + [(16, 0), (16, 0), (16, 1)] + rest[len(rest) // 2:] + reversed_walk(a[5:9]) + random_walk(rng, 5, short)
    walks = [a, [(1, 0)], b, random_walk(rng, 2, short), reversed_walk(b), random_walk(rng, 3, short), c, list(a)]
    return PathGraph(labels, walks)


# ---- the cases of tangle_small: path lists, endmarkers, reads ------------------------------------------------------------------------------

STRIDE = 16                                        # K of the seeds, which the reads are cut around; the GPU tests hold it against the library's
ENDMARKERS = (0, 36, 65)                           # the usual one, another byte no path holds, and one that is also a base
ORDER_NAMES = ("all", "reversed", "subset", "duplicate", "single")


def orders(graph):
    """The path lists by name: the ids in order, reversed, every second id plus the one-step path, a list that names two ids twice, and the
    one-step path alone (a text of label + 1 = 2 bytes)."""
    ids = list(range(graph.paths()))
    return {"all": ids, "reversed": ids[::-1], "subset": ids[0::2] + [ONE_STEP_PATH], "duplicate": ids + [ids[-1], ids[0]], "single": [ONE_STEP_PATH]}


def reads_across(graph, order, endmarker, most=4, flank=20):
    """Reads that run over a path's end: the last bases of a path of `order` followed by the first of the next -- with nothing between them,
    with the endmarker byte, and with a literal A (where the endmarker is 65 these two are one read, and it occurs)."""
    out = []
    for k in range(1, min(len(order), most + 1)):
        head, tail = graph.row_text(order[k - 1])[-flank:], graph.row_text(order[k])[:flank]
        for gap in dict.fromkeys((b"", bytes([endmarker]), b"A")):
            out.append(head + gap + tail)
    return out


def case_reads(graph, order, endmarker):
    """The reads of one case: seed_expect.reads_of over the bases of the first two paths of the list without their endmarkers, the whole
    200-base label and its reverse complement, and the reads across path ends."""
    base = b"".join(graph.row_text(p) for p in order[:2])
    long_label = graph.labels[LONG_NODE]
    return E.reads_of(base, STRIDE) + [long_label, reverse_complement(long_label)] + reads_across(graph, order, endmarker)


class Case:
    """One (path list, endmarker) of a graph with everything the yardsticks say about it, computed once and never written to."""

    def __init__(self, graph, order, endmarker):
        self.graph, self.order, self.endmarker = graph, list(order), endmarker
        self.text, self.bounds = graph.text(order, endmarker), graph.bounds(order)
        self.sa = F.suffix_array(self.text)
        self.tags = graph.tags(order)
        self.sa_tags = self.tags[self.sa.astype(np.int64)]
        self.reads = case_reads(graph, order, endmarker)
        self._seeds = None
        for a in (self.sa, self.tags, self.sa_tags):
            a.setflags(write=False)
        assert self.tags.size == len(self.text) == self.bounds[-1]

    def segment_of(self, y):
        return int(np.searchsorted(np.asarray(self.bounds), y, side="right")) - 1

    def seeds(self):
        """[(read index, start, end, strand, lo, hi)] of both strands of every read, min_length 1."""
        if self._seeds is None:
            self._seeds = [(k,) + seed for k, read in enumerate(self.reads) for strand in (E.FORWARD, E.REVERSE) for seed in E.expected(self.text, self.sa, read, strand)]
        return self._seeds

    def seeds_in_two_segments(self):
        """Seeds with hits in more than one segment."""
        return [s for s in self.seeds() if len({self.segment_of(int(p)) for p in self.sa[s[4]:s[5]]}) > 1]

    def seeds_over_a_path_end(self):
        """(seed, hit) whose occurrence starts in one segment and ends in another: it runs through an endmarker byte."""
        return [(s, int(p)) for s in self.seeds() for p in self.sa[s[4]:s[5]] if self.segment_of(int(p)) != self.segment_of(int(p) + s[2] - s[1] - 1)]

    def reads_without_seeds(self):
        """Reads of at least one byte without a seed on either strand."""
        with_seeds = {s[0] for s in self.seeds()}
        return [k for k, read in enumerate(self.reads) if read and k not in with_seeds]


PERIODIC_READ = b"ACACAC" + b"G" + b"ACACAC"


def periodic(reps):
    """One node AC; path k visits it reps[k] times: the text is b"AC" * r + endmarker per path."""
    return PathGraph({1: b"AC"}, [[(1, 0)] * int(r) for r in reps])


def periodic_matches(reps, min_length=5):
    """The matches of PERIODIC_READ with this min_length: ACACAC at x = 0 and at x = 7, each at every even y of a path that leaves room:
    2 (r - 2) for a path of r >= 3 repeats."""
    assert min_length in (5, 6)
    return sum(2 * (r - 2) for r in reps if r >= 3)


def periodic_reps_for(matches):
    """A list of repeats with exactly `matches` matches of PERIODIC_READ: a first path of 120 repeats (236 matches, more than 128 of them
    inside a window of 400 bases), a 3-repeat and a 2-repeat path (2 matches and none), one of 70 and a last one that makes up the rest."""
    rest = matches - periodic_matches([120, 3, 2, 70])
    assert rest >= 2 and rest % 2 == 0, "no such list for this count"
    reps = [120, 3, 2, 70, rest // 2 + 2]
    assert periodic_matches(reps) == matches
    return reps


def window_starts(matches, bounds, max_gap):
    """For every match i of an item (sorted by (y, x)) the index of the first j with y_j >= low(i) = max(y_i - max_gap, start of i's segment):
    the lower end of the window the DP reads for i.  It never decreases."""
    ys = np.array([m[0] for m in matches], dtype=np.int64)
    starts = np.asarray(bounds, dtype=np.int64)[np.searchsorted(np.asarray(bounds, dtype=np.int64), ys, side="right") - 1]
    return np.searchsorted(ys, np.maximum(ys - max_gap, starts), side="left")


def window_sizes(matches, bounds, max_gap):
    """The matches in the window of every i: those from its lower end up to i."""
    return np.arange(len(matches), dtype=np.int64) - window_starts(matches, bounds, max_gap)
