"""Yardsticks for the FM-index queries, numpy only and without the library.  A pattern P occurs at position i of a text T when
T.startswith(P, i); its occurrences, looked up in the suffix array of tests/tags_expect.py (the brute-force sort), are one stretch of rows
[lo, hi) -- the suffixes that start with P stand together -- and the located row is sa[lo:hi] exactly: SA is unique.  A pattern that does
not occur has (0, 0); the empty pattern occurs at every position of the text: (0, n)."""
import numpy as np

import sa_expect as A
import tags_expect as T


def occurrences_slow(text, p):
    """The definition: startswith at every position."""
    text, p = bytes(text), bytes(p)
    return np.array([i for i in range(len(text)) if text.startswith(p, i)], dtype=np.int64)


def occurrences(text, p):
    """The same positions, ascending, by narrowing the candidates byte by byte (test_fm_cpu.py holds it against occurrences_slow)."""
    t = A.as_text(text)
    p = np.frombuffer(bytes(p), dtype=np.uint8)
    at = np.arange(max(min(t.size - p.size + 1, t.size), 0), dtype=np.int64)
    for j in range(p.size):
        if at.size == 0:
            break
        at = at[t[at + j] == p[j]]
    return at


def sa_range(sa, occ):
    """(lo, hi) of the rows of `sa` that hold the positions `occ`; they must stand together."""
    if len(occ) == 0:
        return 0, 0
    sa = np.asarray(sa).astype(np.int64)
    isa = np.empty(sa.size, dtype=np.int64)
    isa[sa] = np.arange(sa.size)
    rows = isa[np.asarray(occ, dtype=np.int64)]
    lo, hi = int(rows.min()), int(rows.max()) + 1
    assert hi - lo == len(occ), "the suffixes that start with a pattern do not stand together: not a suffix array"
    return lo, hi


def expected(text, sa, patterns):
    """(ranges int64[m, 2], rows: the exact SA slice of every pattern) for a list of patterns."""
    ranges = np.zeros((len(patterns), 2), dtype=np.int64)
    rows = []
    sa = np.asarray(sa)
    for k, p in enumerate(patterns):
        lo, hi = sa_range(sa, occurrences(text, p))
        ranges[k] = lo, hi
        rows.append(sa[lo:hi].astype(np.uint64))
    return ranges, rows


def text_patterns(text):
    """The patterns of the text-level tests: the empty one; substrings at every 7th position of lengths 1, 2, 3 and 9, so that neighbours in
    a wave differ in length; prefixes, suffixes (the last-byte rule), the whole text, the text and one byte more; three that hold bytes
    most texts lack.  The batch is never a multiple of 64."""
    text = bytes(text)
    n = len(text)
    patterns = [b""]
    for at in range(0, n, 7):
        for length in (1, 2, 3, 9):
            if at + length <= n:
                patterns.append(text[at:at + length])
    patterns += [text[:1], text[:3], text[-1:], text[-2:], text[-5:], text, text + b"A", b"\0", b"A\0", b"ZZ"]
    patterns.insert(len(patterns) // 2, text[: min(n, 77)])                   # a long lane between short ones
    if len(patterns) % 64 == 0:
        patterns.append(b"A")
    return patterns


def suffix_array(text):
    return T.suffix_array(bytes(text))
