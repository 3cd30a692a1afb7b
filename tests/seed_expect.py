"""Yardsticks for the seeds of reads on the FM-index, numpy only and without the library.  For a read P[0, L) and a text T, the
start of the end e in 1 .. L is the smallest s <= e such that P[s:e] occurs in T (`P[s:e] in T`); a seed is an occurring substring of the
read that no longer occurring substring of the read contains.  The rule the library applies -- [s(e), e) is a seed when e == L or
s(e + 1) > s(e) -- is held against that containment definition by tests/test_seeds_cpu.py.  The SA range of a seed is fm_expect's: its
occurrences looked up in the brute-force suffix array."""
import numpy as np

import fm_expect as F

FORWARD, REVERSE, BOTH = 1, 2, 3

_COMPLEMENT = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in (("A", "T"), ("C", "G"), ("G", "C"), ("T", "A")):
    _COMPLEMENT[ord(_a)] = _COMPLEMENT[ord(_a.lower())] = ord(_b)


def reverse_complement(read):
    """support::reverse_complement (reference src/support.rs:87-110): A/C/G/T in either case to the upper-case complement, anything else N."""
    return _COMPLEMENT[np.frombuffer(bytes(read), dtype=np.uint8)[::-1]].tobytes()


def strand_read(read, strand):
    return reverse_complement(read) if strand == REVERSE else bytes(read)


def starts_slow(text, read):
    """The definition, end by end: s[e] for e in 0 .. L (s[0] == 0)."""
    text, read = bytes(text), bytes(read)
    return [next(s for s in range(e + 1) if read[s:e] in text) for e in range(len(read) + 1)]


def starts(text, read):
    """The same starts, using that they never decrease: a substring of an occurring string occurs."""
    text, read = bytes(text), bytes(read)
    out, s = [0], 0
    for e in range(1, len(read) + 1):
        while read[s:e] not in text:
            s += 1
        out.append(s)
    return out


def seeds_by_containment(text, read, min_length=1):
    """The slow definition: the occurring substrings [s, e) of the read, e > s, that no other occurring substring contains; by end."""
    text, read = bytes(text), bytes(read)
    L = len(read)
    occurring = {(s, e) for e in range(1, L + 1) for s in range(e) if read[s:e] in text}
    kept = [(s, e) for s, e in occurring if not any((a, b) != (s, e) and a <= s and e <= b for a, b in occurring)]
    return sorted((s, e) for s, e in kept if e - s >= max(min_length, 1))


def seeds_by_rule(start, L, min_length=1):
    """The rule over the starts s[0 .. L]."""
    return [(start[e], e) for e in range(1, L + 1) if e - start[e] >= max(min_length, 1) and (e == L or start[e + 1] > start[e])]


def per_end_steps(text, read):
    """Backward steps of one search per end: e - s(e) that succeed, and the failing one where a byte stands in front of the match and the
    text holds that byte (a byte the text lacks ends a search without a step)."""
    text, read = bytes(text), bytes(read)
    present = set(text)
    s = starts(text, read)
    return sum(e - s[e] + (1 if s[e] > 0 and read[s[e] - 1] in present else 0) for e in range(1, len(read) + 1))


def anchored_steps_of_matching_read(L, K):
    """What the anchors cost for a read that occurs as a whole: every anchor reads back to the start of the read."""
    return sum(L - j * K for j in range(-(-L // K)))


def expected(text, sa, read, strand):
    """The seeds of one strand of a read as (start, end, strand, lo, hi), all of them (min_length 1)."""
    p = strand_read(read, strand)
    out = []
    for s, e in seeds_by_rule(starts(text, p), len(p)):
        lo, hi = F.sa_range(sa, F.occurrences(text, p[s:e]))
        out.append((s, e, strand, lo, hi))
    return out


def strands_of(strands):
    return [t for t in (FORWARD, REVERSE) if strands & t]


def reads_of(text, K=16, rounds=10, seed=41):
    """The reads of the text-level tests: pieces of the text put together -- so that a read holds several seeds -- of the lengths 0, 1,
    K - 1, K, K + 1, 2K + 1 and 77 as neighbours; reads with a byte the text lacks at the first, a middle and the last position and one of
    such bytes only (where the text lacks a byte); the text itself.  Never a multiple of 64 of them."""
    text = bytes(text)
    rng = np.random.default_rng(seed)

    def pieces(length):
        out = b""
        while len(out) < length:
            if text:
                k = int(rng.integers(1, min(len(text), 24) + 1))
                at = int(rng.integers(0, len(text) - k + 1))
                out += text[at:at + k]
            else:
                out += bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=8))
        return out[:length]

    reads = [pieces(length) for _ in range(rounds) for length in (0, 1, K - 1, K, K + 1, 2 * K + 1, 77)]
    lack = next((b for b in (ord("Z"), 255, 1, ord("N")) + tuple(range(256)) if b not in set(text)), None)
    if lack is not None:
        base = bytearray(pieces(2 * K + 1))
        for at in (0, K, 2 * K):
            r = bytearray(base)
            r[at] = lack
            reads.append(bytes(r))
        reads.append(bytes([lack]) * 5)
    reads.append(text)
    if len(reads) % 64 == 0:
        reads.append(pieces(3))
    return reads
