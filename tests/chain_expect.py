"""Yardstick for the chains of seeds, numpy only and without the library: the definition of include/gbwt_hip.h, "Chains of
seeds", restated.  Seeds come from seed_expect.expected, their hits from the brute-force suffix array.

An item is one (read, strand); every hit p of a seed [s, e) of it is a match (y = p, x = s, w = e - s), the matches ordered by (y, x).  j may
precede i when both have one segment, dy = y_i - y_j and dx = x_i - x_j are in 1 .. max_gap and d = |dy - dx| <= max_skew;
c(j, i) = f(j) + min(w_i, dx, dy) - gap_cost * d; f(i) = w_i unless some c(j, i) > w_i: then the largest c and the largest j that attains it.
Peeling visits by (f descending, index ascending); an unused match walks its predecessors until none is left (base 0) or the next one is
used (base = its f); score = f(head) - base; reported when score >= max(min_score, 1)."""
import numpy as np

import seed_expect as E

DEFAULT_GAP, DEFAULT_SKEW = 5000, 500
NONE = -1


def options(max_gap=0, max_skew=0, gap_cost=1, min_score=1):
    """(max_gap, max_skew, gap_cost, min_score) as the arithmetic takes them."""
    return (max_gap or DEFAULT_GAP, max_skew or DEFAULT_SKEW, gap_cost, max(min_score, 1))


def matches_of(text, sa, read, strand, min_length=1, max_occurrences=1 << 20):
    """The matches of one item, sorted by (y, x): [(y, x, w)]."""
    out = []
    for s, e, _, lo, hi in E.expected(text, sa, read, strand):
        if e - s >= max(min_length, 1) and hi - lo <= max_occurrences:
            out += [(int(p), s, e - s) for p in sa[lo:hi]]
    assert len(set((y, x) for y, x, _ in out)) == len(out)                       # two matches of an item never share (y, x)
    return sorted(out)


def segments(ys, bounds):
    """The k with bounds[k] <= y < bounds[k + 1]; 0 without bounds."""
    ys = np.asarray(ys, dtype=np.int64)
    if bounds is None:
        return np.zeros(ys.size, dtype=np.int64)
    return np.searchsorted(np.asarray(bounds, dtype=np.int64), ys, side="right") - 1


def dp_slow(y, x, w, seg, opts):
    """The definition in plain loops: (f, pred, admissible pairs)."""
    max_gap, max_skew, gap_cost, _ = opts
    n = len(y)
    f, pred, pairs = [0] * n, [NONE] * n, 0
    for i in range(n):
        f[i] = w[i]
        best = None
        for j in range(i):
            dy, dx = y[i] - y[j], x[i] - x[j]
            if seg[j] != seg[i] or not 1 <= dy <= max_gap or not 1 <= dx <= max_gap or abs(dy - dx) > max_skew:
                continue
            pairs += 1
            c = f[j] + min(w[i], dx, dy) - gap_cost * abs(dy - dx)
            if c > w[i] and (best is None or c >= best):
                best, pred[i] = c, j
        if best is not None:
            f[i] = best
    return f, pred, pairs


def dp(y, x, w, seg, opts):
    """The same with one numpy expression per i."""
    max_gap, max_skew, gap_cost, _ = opts
    y, x, w, seg = (np.asarray(a, dtype=np.int64) for a in (y, x, w, seg))
    n = y.size
    f, pred, pairs = w.copy(), np.full(n, NONE, dtype=np.int64), 0
    for i in range(1, n):
        dy, dx = y[i] - y[:i], x[i] - x[:i]
        d = np.abs(dy - dx)
        ok = (seg[:i] == seg[i]) & (dy >= 1) & (dy <= max_gap) & (dx >= 1) & (dx <= max_gap) & (d <= max_skew)
        pairs += int(ok.sum())
        c = f[:i] + np.minimum(w[i], np.minimum(dx, dy)) - gap_cost * d
        keep = ok & (c > w[i])
        if keep.any():
            best = c[keep].max()
            f[i], pred[i] = best, np.flatnonzero(keep & (c == best))[-1]
    return f.tolist(), pred.tolist(), pairs


def peel(f, pred):
    """Every chain of an item in peeling order, reported or not: [(score, base, members ascending)]."""
    used = [False] * len(f)
    chains = []
    for i in sorted(range(len(f)), key=lambda k: (-f[k], k)):
        if used[i]:
            continue
        members, at, base = [], i, 0
        while True:
            used[at] = True
            members.append(at)
            p = pred[at]
            if p == NONE:
                break
            if used[p]:
                base = f[p]
                break
            at = p
        chains.append((f[i] - base, base, members[::-1]))
    assert all(used)
    return chains


def item_chains(matches, seg, opts, strand):
    """The reported chains of one item: ([(text_start, text_end, read_start, read_end, score, members, strand, path)], [[(y, x, w)]], pairs)."""
    y, x, w = ([m[k] for m in matches] for k in range(3))
    f, pred, pairs = dp(y, x, w, seg, opts)
    rows, members_of = [], []
    for score, _, members in peel(f, pred):
        if score < opts[3]:
            continue
        first, last = members[0], members[-1]
        rows.append((y[first], y[last] + w[last], x[first], x[last] + w[last], score, len(members), strand, int(seg[last])))
        members_of.append([matches[k] for k in members])
    return rows, members_of, pairs


def expected_rows(text, sa, reads, min_length=1, strands=E.BOTH, max_occurrences=1 << 20, max_gap=0, max_skew=0, gap_cost=1, min_score=1, max_matches=0, bounds=None):
    """What FMIndex.chains returns, as lists, and the counts of last_chain_info: a dict."""
    opts = options(max_gap, max_skew, gap_cost, min_score)
    out = dict(read_offsets=[0], chains=[], match_offsets=[0], matches=[], items=0, n_matches=0, pairs=0, skipped_items=0)
    for read in reads:
        for strand in E.strands_of(strands):
            out["items"] += 1
            matches = matches_of(text, sa, read, strand, min_length, max_occurrences)
            if max_matches and len(matches) > max_matches:
                out["skipped_items"] += 1
                continue
            out["n_matches"] += len(matches)
            rows, members_of, pairs = item_chains(matches, segments([m[0] for m in matches], bounds), opts, strand)
            out["pairs"] += pairs
            for row, members in zip(rows, members_of):
                out["chains"].append(row)
                out["matches"] += members
                out["match_offsets"].append(len(out["matches"]))
        out["read_offsets"].append(len(out["chains"]))
    return out
