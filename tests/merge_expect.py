"""The merge of two bidirectional GBWT indexes, step by step in pure Python: the recurrence the kernels of csrc/merge.hip run,
over the decoded records of two indexes.

  P_X(w, v)  = visits of w in X whose predecessor is below v: 0 from the endmarker; the stored offset of v -> w where X has that edge; else
               the stored offset of u -> w for the smallest predecessor u > v of w -- the predecessors of w are the flipped nonzero
               successors of flip(w) --; else the length of w's record.
  cross walk = every sequence of W (the input with fewer visits, b on a tie) is followed in W with LF and in R with the successor forced:
               c' = P_R(w, v) + occurrences of w among the first c entries of R's body of v.
  interleave = W's visit j lies at j + c_j, R's visit i at i + |{j : c_j <= i}|.
  offsets    = P_a(w, v) + P_b(w, v); 0 to the endmarker and in the endmarker's record.

Nothing here sorts by prefix; tests/test_merge_cpu.py holds it against the brute-force builder over the concatenated paths."""
import bisect


def _varint(data, at):
    value, shift = 0, 0
    while True:
        b = int(data[at])
        at += 1
        value += (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return value, at


class Index:
    """Decoded records: edges[v] = [(successor, offset)], body[v] = [successor of every visit]; v = 0 is the endmarker."""

    def __init__(self, data, starts, sequences, alphabet_offset, alphabet_size):
        self.sequences, self.alphabet_offset, self.alphabet_size = sequences, alphabet_offset, alphabet_size
        self.edges, self.body = {}, {}
        bounds = [int(s) for s in starts] + [len(data)]
        for r in range(len(bounds) - 1):
            at, end = bounds[r], bounds[r + 1]
            if at >= end:
                continue
            sigma, at = _varint(data, at)
            if sigma == 0:
                continue
            edges, node = [], 0
            for _ in range(sigma):
                delta, at = _varint(data, at)
                offset, at = _varint(data, at)
                node += delta
                edges.append((node, offset))
            body = []
            while at < end:
                if sigma >= 255:
                    value, at = _varint(data, at)
                    length, at = _varint(data, at)
                    length += 1
                else:
                    b = int(data[at])
                    at += 1
                    value, length = b % sigma, b // sigma + 1
                    if length == 256 // sigma:
                        extra, at = _varint(data, at)
                        length += extra
                body += [edges[value][0]] * length
            v = 0 if r == 0 else r + alphabet_offset
            self.edges[v], self.body[v] = edges, body
        self.visits = sum(len(b) for v, b in self.body.items() if v != 0)

    @classmethod
    def of(cls, synth):
        return cls(synth.data(), synth.starts(), synth.sequences, synth.alphabet_offset, synth.alphabet_size)

    def length(self, v):
        return len(self.body.get(v, ()))

    def offset(self, v, w):
        for node, offset in self.edges.get(v, ()):
            if node == w:
                return offset
        return None

    def lf(self, v, i):
        """(w, offset in w) behind position i of v; w = 0: the sequence ends."""
        w = self.body[v][i]
        return w, (self.offset(v, w) if v != 0 else 0) + self.body[v][:i].count(w)

    def pred_rank(self, w, v):
        """P(w, v); v = 1 stands for "below every node" (only the starts are below it)."""
        if v == 0 or w == 0 or self.length(w) == 0:
            return 0
        stored = self.offset(v, w) if v >= 2 else None
        if stored is not None:
            return stored
        above = [s ^ 1 for s, _ in self.edges.get(w ^ 1, ()) if s != 0 and (s ^ 1) > v]
        return self.offset(min(above), w) if above else self.length(w)


def merge(a, b):
    """(edges, body, walked) of the index of a's sequences followed by b's: edges[v] = [(successor, offset)], body[v] = [successors]."""
    walk_b = b.visits <= a.visits
    W, R = (b, a) if walk_b else (a, b)
    cross = {v: [None] * len(body) for v, body in W.body.items()}
    if 0 in cross:
        cross[0] = [R.sequences if walk_b else 0] * len(cross[0])
    for x in range(W.sequences):
        v, i = W.lf(0, x)
        if v == 0:
            continue
        c = R.pred_rank(v, 1) if walk_b else 0
        while True:
            cross[v][i] = c
            w, j = W.lf(v, i)
            if w == 0:
                break
            stored = R.offset(v, w) if R.length(v) else None
            c = stored + R.body[v][:c].count(w) if stored is not None else R.pred_rank(w, v)
            v, i = w, j
    for v, ranks in cross.items():
        assert None not in ranks, (v, ranks)
        assert ranks == sorted(ranks), (v, ranks)            # within a record the cross ranks do not decrease
    body = {}
    for v in sorted(set(W.body) | set(R.body)):
        ranks, mine, theirs = cross.get(v, []), W.body.get(v, []), R.body.get(v, [])
        out = [None] * (len(mine) + len(theirs))
        for j, c in enumerate(ranks):
            out[j + c] = mine[j]
        for i, succ in enumerate(theirs):
            out[i + bisect.bisect_right(ranks, i)] = succ
        assert None not in out, (v, out)
        body[v] = out
    edges = {}
    for v, out in body.items():
        edges[v] = [(w, 0 if v == 0 or w == 0 else a.pred_rank(w, v) + b.pred_rank(w, v)) for w in sorted(set(out))]
    return edges, body, (1 if walk_b else 0)


def special_pairs():
    """(name, paths of a, paths of b): the smallest shapes at which a stage of the merge can go wrong (tests/test_gpu_merge.py)."""
    pairs = []
    for name, pa, pb in (("edge-missing-predecessor-above", [[2, 4, 6]], [[2, 6]]), ("edge-missing-node-absent", [[2, 4, 6]], [[8, 6]]),
                         ("edge-missing-successor-absent", [[2, 4, 6]], [[2, 10]])):
        pairs += [(name, pa, pb), (name + "-swapped", pb, pa)]
    pairs.append(("orientation-pairs", [[2, 6], [3, 6]], [[2, 6], [3, 6], [4, 6]]))
    pairs.append(("orientation-pairs-swapped", [[2, 6], [3, 6], [4, 6]], [[2, 6], [3, 6]]))
    pairs.append(("orientation-pairs-reverse", [[2, 7], [3, 7]], [[2, 7], [3, 7], [4, 7]]))
    pairs.append(("orientation-pairs-reverse-swapped", [[2, 7], [3, 7], [5, 7]], [[2, 7], [3, 7]]))
    pairs.append(("ties", [[2, 4, 6, 8, 10] * 8] * 200, [[2, 4, 6, 8, 10] * 8] * 200))
    pairs.append(("own-reverse", [[2, 3], [4, 6, 7, 5]], [[2, 3], [4, 6, 7, 5]]))
    pairs.append(("long-run", [[2] * 300], [[2] * 4096]))
    pairs.append(("disjoint-down", [[200, 202]], [[2, 4]]))
    pairs.append(("disjoint-up", [[2, 4]], [[200, 202]]))
    pairs.append(("long-deltas", [[2, 2 * 100001]], [[2 * 100001 + 1, 3]]))
    pairs.append(("long-deltas-swapped", [[2 * 100001 + 1, 3]], [[2, 2 * 100001]]))
    return pairs


def hub_pair(k):
    """Node 2 with k successors, the even ones in a and the odd ones in b, twice each."""
    rows = [[2, 2 * (2 + i)] for i in range(k)]
    return [r for r in rows[0::2] for _ in range(2)], [r for r in rows[1::2] for _ in range(2)]
