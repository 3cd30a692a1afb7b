"""The removal of paths from a GBWT index, step by step in pure Python: the deletion the kernels of csrc/remove.hip run, over
the decoded records of the index (merge_expect.Index).

  positions  = all positions of all records as one array; record r owns [first[r], first[r] + len[r]), the endmarker's comes first.
  marks      = position s of the endmarker's record and every position LF reaches from the start of sequence s, for every removed s.
  M          = exclusive prefix sum of the marks, with one entry past the last position.
  compaction = a kept position i moves to i - M[i]; the bodies keep their order.
  offsets    = P' = P - (M[first[w] + P] - M[first[w]]) for a kept edge v -> w with the old stored offset P; 0 to the endmarker and in
               the endmarker's record.

Nothing here sorts by prefix; tests/test_remove_cpu.py holds it against the brute-force builder over the kept paths.  The shapes of
tests/test_gpu_remove.py are generated here as well."""
import merge_expect as MX


def sequences_of(path_ids, bidirectional):
    """The sequence ids of the paths: 2p and 2p + 1 in a bidirectional index, p in a unidirectional one."""
    return [s for p in path_ids for s in ((2 * p, 2 * p + 1) if bidirectional else (p,))]


def remove(index, removed_sequences):
    """(edges, body, sequences, removed_steps) of the index without the sequences: edges[v] = [(successor, offset)], body[v] = [successors];
    records without a kept visit are absent."""
    nodes = sorted(index.body)                                   # 0, the endmarker, first
    first, total = {}, 0
    for v in nodes:
        first[v] = total
        total += len(index.body[v])
    mark = [0] * (total + 1)
    for s in removed_sequences:
        assert not mark[first[0] + s]
        mark[first[0] + s] = 1
        v, i = index.lf(0, s)
        steps = 0
        while v != 0:
            assert steps < total and not mark[first[v] + i]     # every position belongs to one sequence
            mark[first[v] + i] = 1
            v, i = index.lf(v, i)
            steps += 1
    M = [0] * (total + 2)
    for i in range(total + 1):
        M[i + 1] = M[i] + mark[i]
    body = {}
    for v in nodes:
        kept = [w for i, w in enumerate(index.body[v]) if not mark[first[v] + i]]
        if kept:
            body[v] = kept
    edges = {}
    for v, kept in body.items():
        edges[v] = []
        for w in sorted(set(kept)):
            offset = 0
            if v != 0 and w != 0:
                P = index.offset(v, w)                           # the edge exists: a kept visit took it
                offset = P - (M[first[w] + P] - M[first[w]])
            edges[v].append((w, offset))
    return edges, body, index.sequences - len(removed_sequences), M[total] - len(removed_sequences)


def _varint(value):
    out = bytearray()
    while value >= 0x80:
        out.append((value & 0x7F) | 0x80)
        value >>= 7
    out.append(value)
    return bytes(out)


def encode(edges, body, sequences):
    """(data, starts, alphabet_offset, alphabet_size) of decoded records, as the construction writes them: the alphabet of the visited
    nodes, an unvisited node the one byte 0, maximal runs."""
    visited = [v for v in body if v != 0]
    alphabet_offset, alphabet_size = (min(visited) - 1, max(visited) + 1) if visited else (0, 1)
    data, starts = bytearray(), []
    for r in range(alphabet_size - alphabet_offset):
        v = 0 if r == 0 else r + alphabet_offset
        starts.append(len(data))
        if v not in body:
            data += _varint(0)
            continue
        sigma = len(edges[v])
        data += _varint(sigma)
        rank, last = {}, 0
        for k, (w, offset) in enumerate(edges[v]):
            data += _varint(w - last) + _varint(offset)
            rank[w], last = k, w
        at = 0
        while at < len(body[v]):
            end = at
            while end < len(body[v]) and body[v][end] == body[v][at]:
                end += 1
            value, length = rank[body[v][at]], end - at
            if sigma >= 255:
                data += _varint(value) + _varint(length - 1)
            else:
                threshold = 256 // sigma
                if length < threshold:
                    data.append(value + sigma * (length - 1))
                else:
                    data.append(value + sigma * (threshold - 1))
                    data += _varint(length - threshold)
            at = end
    assert sequences > 0 or not body
    return bytes(data), starts, alphabet_offset, alphabet_size


def remove_paths(synth, path_ids):
    """(data, starts, header) of the Synth index without the paths: header as tests/test_gpu_merge.py compares it."""
    index = MX.Index.of(synth)
    edges, body, sequences, _ = remove(index, sequences_of(path_ids, synth.bidirectional))
    data, starts, alphabet_offset, alphabet_size = encode(edges, body, sequences)
    visits = sum(len(b) for v, b in body.items() if v != 0)
    return data, starts, (sequences, sequences + visits, alphabet_offset, alphabet_size, synth.bidirectional)


def special_removals():
    """(name, paths, removed path ids, bidirectional): the smallest shapes at which a stage of the removal can go wrong."""
    same = [2, 4, 6, 8]
    shapes = [
        ("nothing", [[2, 4, 6], [2, 6]], [], True),
        ("all", [[2, 4, 6], [2, 6]], [0, 1], True),
        ("only-empty-kept", [[], [2, 4], []], [1], True),
        ("only-empty-removed", [[], [2, 4], []], [0, 2], True),
        ("identical-first", [same, same, same], [0], True),
        ("identical-middle", [same, same, same], [1], True),
        ("identical-last", [same, same, same], [2], True),
        ("five-visits-of-one-node", [[4, 6, 4, 8, 4, 6, 4, 4], [4, 6, 8], [8, 4]], [0], True),
        ("alone-on-the-smallest", [[2, 6, 8], [6, 8, 10], [8, 6]], [0], True),
        ("alone-on-the-largest", [[4, 6, 8], [6, 8, 20], [8, 6]], [1], True),
        ("interior-record-emptied", [[2, 8, 12], [2, 12], [12, 2]], [0], True),
        ("unidirectional-first", [[2, 4, 2, 4, 2, 6], [4, 2]], [0], False),
        ("unidirectional-second", [[2, 4, 2, 4, 2, 6], [4, 2]], [1], False),
    ]
    for n in (64, 65, 256, 257):                                 # a record of n visits: the lane / workgroup boundary of the decode and its LDS tile
        paths = [[2, 4 + 2 * (k % 3), 12] for k in range(n)]
        shapes.append((f"record-of-{n}", paths, [0, n // 2, n - 1], True))
    return shapes


def hub(k):
    """Node 2 with k successors, twice each (merge_expect.hub_pair joined), and the last spoke as the paths to remove."""
    a, b = MX.hub_pair(k)
    paths = list(a) + list(b)
    last = max(p[1] for p in paths)
    return paths, [i for i, p in enumerate(paths) if p[1] == last]
