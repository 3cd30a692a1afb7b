"""Yardsticks for suffix arrays, numpy only and without the library.  The order: the suffixes of a text of bytes as unsigned byte strings
compared to the end of the text, a suffix that is a proper prefix of another first (tags_expect.suffix_array states the same by brute force).

doubling(text): an independent prefix doubling with np.lexsort -- a second algorithm, for texts of some 100 000 bytes (300 060 bytes in about
1 s; 3 000 060 take 11 s, so it is not used there).
check(text, sa): the linear certificate, sound and complete for this order (0.4 s at 3 M bytes): sa is a permutation, and for neighbours
a = sa[i], b = sa[i + 1] either T[a] < T[b], or T[a] == T[b] and isa[a + 1] < isa[b + 1] with isa[n] = -1.  Sound: by induction over the
length of the common prefix the suffix at a is smaller than the one at b -- the first bytes decide, or they agree and the rest, shorter by
one, is ordered by sa itself (isa[n] = -1: the empty rest is the smallest).  Complete: the true array satisfies it."""
import numpy as np


def as_text(text):
    return np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, dtype=np.uint8)


def doubling(text):
    t = as_text(text).astype(np.int64)
    n = t.size
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    rank = t + 1                                      # 0 is "past the end"
    h = 1
    while True:
        second = np.zeros(n, dtype=np.int64)
        if h < n:
            second[: n - h] = rank[h:]
        order = np.lexsort((second, rank))
        r, s = rank[order], second[order]
        new = np.empty(n, dtype=np.int64)
        new[0] = 1
        new[1:] = 1 + np.cumsum((r[1:] != r[:-1]) | (s[1:] != s[:-1]))
        rank = np.empty(n, dtype=np.int64)
        rank[order] = new
        if new[-1] == n:
            return order.astype(np.uint64)
        h *= 2


def check(text, sa):
    """None when sa is the suffix array of text, else a sentence that says what is wrong."""
    t = as_text(text).astype(np.int64)
    n = t.size
    sa = np.asarray(sa)
    if sa.shape != (n,):
        return f"shape {sa.shape} for a text of {n} bytes"
    if n == 0:
        return None
    if int(sa.max()) >= n:
        return f"value {int(sa.max())} out of range"
    s = sa.astype(np.int64)
    seen = np.zeros(n, dtype=bool)
    seen[s] = True
    if not seen.all():
        return f"not a permutation: {int(np.flatnonzero(~seen)[0])} is missing"
    isa = np.empty(n + 1, dtype=np.int64)
    isa[s] = np.arange(n)
    isa[n] = -1
    a, b = s[:-1], s[1:]
    ok = (t[a] < t[b]) | ((t[a] == t[b]) & (isa[a + 1] < isa[b + 1]))
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        return f"suffixes {int(a[i])} and {int(b[i])} at places {i}, {i + 1} are out of order"
    return None


def bwt(text, sa, sentinel=0):
    """BWT[i] = T[SA[i] - 1], the sentinel byte where SA[i] == 0."""
    t = as_text(text)
    s = np.asarray(sa).astype(np.int64)
    out = t[s - 1].copy() if t.size else np.zeros(0, dtype=np.uint8)
    out[s == 0] = sentinel
    return out


def runs(values):
    """count_bwt_runs (src/bin/gbz-extract.rs:373-406): entries that differ from the one in front, the first counting as one."""
    values = np.asarray(values)
    return 0 if values.size == 0 else 1 + int(np.count_nonzero(values[1:] != values[:-1]))


def mutated_rows(rows, length, substitutions, endmarker=0, seed=5):
    """A repetitive text: `rows` copies of one random ACGT row of `length` bases, each with `substitutions` bases replaced, an endmarker behind each."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
    base = alphabet[rng.integers(0, 4, size=length)]
    out = np.empty(rows * (length + 1), dtype=np.uint8)
    for r in range(rows):
        row = base.copy()
        at = rng.integers(0, length, size=substitutions)
        row[at] = alphabet[(np.searchsorted(alphabet, row[at]) + rng.integers(1, 4, size=substitutions)) % 4]
        out[r * (length + 1): r * (length + 1) + length] = row
        out[r * (length + 1) + length] = endmarker
    return out.tobytes()


def fibonacci(length):
    a, b = b"A", b"AB"
    while len(b) < length:
        a, b = b, b + a
    return b[:length]


def small_texts():
    """(name, bytes) of the short texts of the text-level tests: around the packed key, zeros, all byte values, periodic texts."""
    rng = np.random.default_rng(3)
    texts = [("empty", b"")] + [(f"len{k}", bytes(rng.integers(65, 68, size=k).astype(np.uint8))) for k in (1, 2, 7, 8, 9)]
    texts.append(("zeros", b"\0\0\0A\0\0"))
    texts.append(("all_bytes", bytes(rng.permutation(np.arange(4099) % 256).astype(np.uint8))))
    texts.append(("ac", b"AC" * 2500))
    texts.append(("fibonacci", fibonacci(4181)))
    texts.append(("a_run", b"A" * 5000 + b"\0"))
    return texts
