"""Yardstick for the alignments of chains, numpy only and without the library: the definition of include/gbwt_hip.h,
"Alignments of chains", restated.  Chains come from chain_expect.expected_rows.

A member (y, x, w) of a chain lies on the diagonal d = y - x; d0 = min d - band, W = max d - min d + 2 band + 1.  H(i, j) for 0 <= i <= L and
j = i + d0 + k, 0 <= k < W; only cells with lo <= j <= hi exist.  H(0, j) = 0; below it the smallest of the diagonal H(i - 1, j - 1) +
(P[i - 1] != T[j - 1]), the insertion H(i - 1, j) + 1 and the deletion H(i, j - 1) + 1 over existing, reachable cells, the direction the first of
the three that attains it.  The result is the smallest H(L, j) at the smallest j; the walk back gives text_start and the CIGAR as run-length
entries (length << 4) | op with I = 1, D = 2, '=' = 7, X = 8."""
import numpy as np

import chain_expect as X
import seed_expect as E

OK, WIDE, NONE = 0, 1, 2
INF = 0xFFFFFFFF
MAX_WIDTH, DEFAULT_WIDTH = 1024, 256
DIAGONAL, INSERTION, DELETION = 0, 1, 2
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
_BIG = 1 << 40


def band_of(members, band):
    """(d0, W) of the members [(y, x, w)] of a chain."""
    ds = [y - x for y, x, _ in members]
    return min(ds) - band, max(ds) - min(ds) + 2 * band + 1


def pack(ops):
    """A list of operations in read order as run-length entries."""
    out = []
    for op in ops:
        if out and out[-1][1] == op:
            out[-1][0] += 1
        else:
            out.append([1, op])
    return [(n << 4) | op for n, op in out]


def cigar_string(entries):
    return "".join(f"{int(v) >> 4}{ {1: 'I', 2: 'D', 7: '=', 8: 'X'}[int(v) & 15]}" for v in entries)


def _trace(P, T, d0, L, H_last, direction_at):
    """The result from row L and the directions: (status, edit_distance, text_start, text_end, entries)."""
    ends = [(h, k) for k, h in enumerate(H_last) if h is not None]
    if not ends:
        return NONE, INF, 0, 0, []
    distance, k = min(ends)
    i, text_end, ops = L, L + d0 + k, []
    while i > 0:
        direction = direction_at(i, k)
        if direction == DIAGONAL:
            j = i + d0 + k
            ops.append(OP_EQ if P[i - 1] == T[j - 1] else OP_X)
            i -= 1
        elif direction == INSERTION:
            ops.append(OP_I)
            i, k = i - 1, k + 1
        else:
            ops.append(OP_D)
            k -= 1
    return OK, distance, d0 + k, text_end, pack(ops[::-1])


def align_slow(P, T, members, band, max_width, lo, hi):
    """The definition in plain loops over the full (L + 1) x W table: (status, width, edit_distance, text_start, text_end, entries)."""
    d0, W = band_of(members, band)
    if W > (max_width or DEFAULT_WIDTH):
        return WIDE, W, INF, 0, 0, []
    L = len(P)
    H = [[None] * W for _ in range(L + 1)]
    D = [[None] * W for _ in range(L + 1)]
    for k in range(W):
        if lo <= d0 + k <= hi:
            H[0][k] = 0
    for i in range(1, L + 1):
        for k in range(W):
            j = i + d0 + k
            if not lo <= j <= hi:
                continue
            candidates = []
            if H[i - 1][k] is not None:                                          # (i - 1, j - 1): the same diagonal
                candidates.append((H[i - 1][k] + (P[i - 1] != T[j - 1]), DIAGONAL))
            if k + 1 < W and H[i - 1][k + 1] is not None:                        # (i - 1, j): the diagonal above
                candidates.append((H[i - 1][k + 1] + 1, INSERTION))
            if k >= 1 and H[i][k - 1] is not None:                               # (i, j - 1): the diagonal below, in this row
                candidates.append((H[i][k - 1] + 1, DELETION))
            if candidates:
                H[i][k], D[i][k] = min(candidates)                               # the smallest value, then the first direction
    return (lambda r: (r[0], W) + r[1:])(_trace(P, T, d0, L, H[L], lambda i, k: D[i][k]))


def align(P, T, members, band, max_width, lo, hi):
    """The same with one numpy expression per row: the deletion chain is a prefix minimum of A(k) - k."""
    d0, W = band_of(members, band)
    if W > (max_width or DEFAULT_WIDTH):
        return WIDE, W, INF, 0, 0, []
    L = len(P)
    Pa, Ta = np.frombuffer(bytes(P), dtype=np.uint8), np.frombuffer(bytes(T), dtype=np.uint8)
    ks = np.arange(W, dtype=np.int64)
    exists = lambda i: (i + d0 + ks >= lo) & (i + d0 + ks <= hi)
    h = np.where(exists(0), 0, _BIG)
    directions = np.zeros((L + 1, W), dtype=np.uint8)
    for i in range(1, L + 1):
        here = exists(i)
        t = Ta[np.clip(i + d0 + ks - 1, 0, max(Ta.size - 1, 0))] if Ta.size else np.zeros(W, dtype=np.uint8)
        diagonal = np.where(h < _BIG, h + (t != Pa[i - 1]), _BIG)
        above = np.append(h[1:], _BIG)
        insertion = np.where(above < _BIG, above + 1, _BIG)
        a = np.where(here, np.minimum(diagonal, insertion), _BIG)
        row = np.where(insertion < diagonal, INSERTION, DIAGONAL)
        chained = np.minimum.accumulate(np.where(a < _BIG, a - ks, _BIG)) + ks
        value = np.where(here & (chained < _BIG // 2), chained, _BIG)
        directions[i] = np.where(value < a, DELETION, row)
        h = value
    last = [None if v >= _BIG else int(v) for v in h]
    return (lambda r: (r[0], W) + r[1:])(_trace(P, T, d0, L, last, lambda i, k: int(directions[i, k])))


def check_alignment(P, T, row, entries):
    """The invariants of an OK alignment (status, width, edit_distance, text_start, text_end): read length, text length, edits, and the replay."""
    _, _, distance, start, end = row[:5]
    i, j, edits = 0, start, 0
    for v in entries:
        n, op = v >> 4, v & 15
        assert n >= 1 and op in (OP_I, OP_D, OP_EQ, OP_X)
        if op in (OP_EQ, OP_X):
            for t in range(n):
                assert (P[i + t] == T[j + t]) == (op == OP_EQ)
            i, j = i + n, j + n
        elif op == OP_I:
            i += n
        else:
            j += n
        edits += n if op != OP_EQ else 0
    assert i == len(P) and j == end and edits == distance
    assert not entries or (entries[0] & 15 != OP_D and entries[-1] & 15 != OP_D)
    assert all((a & 15) != (b & 15) for a, b in zip(entries, entries[1:]))


def expected_rows(text, sa, reads, min_length=1, strands=E.BOTH, max_occurrences=1 << 20, max_gap=0, max_skew=0, gap_cost=1, min_score=1, max_matches=0, band=16, max_width=0,
                  max_alignments=0, bounds=None, form=align):
    """What FMIndex.alignments returns, as lists, and the counts of last_align_info: a dict ("chain_rows": chain_expect.expected_rows of the request)."""
    want = X.expected_rows(text, sa, reads, min_length, strands, max_occurrences, max_gap, max_skew, gap_cost, min_score, max_matches, bounds)
    out = dict(read_offsets=[0], alignments=[], cigar_offsets=[0], cigars=[], items=want["items"], wide=0, unreachable=0, cells=0, chain_rows=want)
    for k, read in enumerate(reads):
        rows = range(want["read_offsets"][k], want["read_offsets"][k + 1])
        for strand in E.strands_of(strands):
            P = read if strand == E.FORWARD else E.reverse_complement(read)
            mine = [c for c in rows if want["chains"][c][6] == strand]
            for c in mine[:max_alignments or None]:
                path = want["chains"][c][7]
                lo, hi = (0, len(text)) if bounds is None else (bounds[path], bounds[path + 1] - 1)
                members = want["matches"][want["match_offsets"][c]:want["match_offsets"][c + 1]]
                status, width, distance, start, end, entries = form(P, text, members, band, max_width, lo, hi)
                out["alignments"].append((start, end, c, distance, width, status, strand, path))
                out["cigars"] += entries
                out["cigar_offsets"].append(len(out["cigars"]))
                out["wide"] += status == WIDE
                out["unreachable"] += status == NONE
                out["cells"] += 0 if status == WIDE else (len(P) + 1) * width
                if status == OK:
                    check_alignment(P, text, (status, width, distance, start, end), entries)
        out["read_offsets"].append(len(out["alignments"]))
    return out
