// fm_seeds.hpp -- the maximal exact matches of a read on the FM-index (include/gbwt_hip.h, "Seeds of reads") as kernels
// (fm_seeds.hip) and a host program (tests/cpp/fm_seeds.cpp) both see them: the strand's view of a read, the longest occurring suffix of a
// prefix, where the anchors of a read stand, and the seed rule.  __host__ __device__, no HIP call, as fm_layout.hpp.
//
// STARTS.  For an end e in 1 .. L of the read P[0, L), s(e) is the smallest s <= e such that P[s, e) occurs in the text (s(e) == e: the
// byte P[e - 1] does not occur).  s never decreases as e grows: a substring of an occurring string occurs.
// SEEDS.  [s(e), e) is a seed when it is long enough and e == L or s(e + 1) > s(e): the occurring substrings of the read that no longer
// occurring substring of the read contains.
// ANCHORS.  The ends L, L - K, L - 2K, .. > 0 are searched first; between two anchors with the same start nothing ends a seed, so only
// the ends between anchors whose starts differ are searched as well (`refined`).
#pragma once

#include <cstdint>

#include "fm_layout.hpp"

namespace gbwt_hip {

#ifndef GBWT_HIP_SEED_STRIDE
#define GBWT_HIP_SEED_STRIDE 16               // tools/seed_bench.py measured 8, 16 and 32
#endif
constexpr uint32_t FM_SEED_STRIDE = GBWT_HIP_SEED_STRIDE;   // K: ends between two anchors of a read
constexpr uint32_t FM_STRAND_FORWARD = 1;     // the read as given
constexpr uint32_t FM_STRAND_REVERSE = 2;     // support::reverse_complement of it (src/support.rs:87-110)

// The complement table of support::reverse_complement as a function: A/C/G/T in either case to the upper-case complement, anything else N
FM_HD uint8_t fm_complement(uint8_t b) {
    switch (b) {
        case 'A': case 'a': return 'T';
        case 'C': case 'c': return 'G';
        case 'G': case 'g': return 'C';
        case 'T': case 't': return 'A';
        default: return 'N';
    }
}

// Byte j of the strand's read, read in place: the reverse strand is comp(P[L - 1 - j])
FM_HD uint8_t fm_strand_byte(const uint8_t *read, uint32_t len, uint32_t strand, uint32_t j) {
    return strand == FM_STRAND_REVERSE ? fm_complement(read[len - 1 - j]) : read[j];
}

// The strands of a request (1 forward, 2 reverse, 3 both): how many, and the t-th of them
FM_HD uint32_t fm_strand_count(uint32_t strands) { return strands == 3 ? 2 : 1; }
FM_HD uint32_t fm_strand_at(uint32_t strands, uint32_t t) { return strands == 3 ? t + 1 : strands; }

// The anchors of a read of L bytes, ascending: rank a of fm_anchor_count(L) stands at the end fm_anchor_end(L, a); the last one is L
FM_HD uint32_t fm_anchor_count(uint32_t L, uint32_t K = FM_SEED_STRIDE) { return L / K + (L % K != 0 ? 1 : 0); }
FM_HD uint32_t fm_anchor_end(uint32_t L, uint32_t a, uint32_t K = FM_SEED_STRIDE) { return L - (fm_anchor_count(L, K) - 1 - a) * K; }
// the end in front of anchor a: the anchor before it, or the virtual one at end 0 with start 0
FM_HD uint32_t fm_anchor_before(uint32_t L, uint32_t a, uint32_t K = FM_SEED_STRIDE) { return a == 0 ? 0 : fm_anchor_end(L, a - 1, K); }
// the ends strictly between that one and anchor a are searched when the two starts differ
FM_HD uint32_t fm_refined_ends(uint32_t end_before, uint32_t start_before, uint32_t end, uint32_t start) { return start == start_before ? 0 : end - end_before - 1; }

// The seed rule.  next_start: s(e + 1), anything where e == L
FM_HD bool fm_is_seed(uint32_t start, uint32_t end, uint32_t L, uint32_t next_start, uint32_t min_length) {
    const uint32_t least = min_length < 1 ? 1 : min_length;
    return end - start >= least && (end == L || next_start > start);
}

// fm_search's loop over the strand's read[0, e), except that it keeps the last non-empty range and where it stood: s = s(e), and [lo, hi)
// = the SA range of read[s, e) in fm_search's coordinates ((0, n) where s == e).  Returns the backward steps taken, the failing one
// included; a byte the text lacks ends the search without a step.
FM_HD uint32_t fm_longest_suffix(const FmLayout &L, const uint16_t *code, const uint32_t *C, const uint8_t *read, uint32_t e, uint32_t strand, uint32_t read_len,
                                 uint32_t &out_s, uint64_t &out_lo, uint64_t &out_hi) {
    uint64_t lo = 0, hi = L.rows;
    uint32_t s = e, steps = 0;
    for (uint32_t j = e; j > 0; j--) {
        const uint16_t c = code[fm_strand_byte(read, read_len, strand, j - 1)];
        if (c == FM_ABSENT) break;
        uint64_t next_lo = lo, next_hi = hi;
        fm_step(L, C, c, next_lo, next_hi);
        steps++;
        if (next_lo >= next_hi) break;
        lo = next_lo;
        hi = next_hi;
        s = j - 1;
    }
    out_s = s;
    out_lo = lo == 0 ? 0 : lo - 1;                                                // SA coordinates: row 0 is no SA row
    out_hi = hi - 1;
    return steps;
}

}  // namespace gbwt_hip
