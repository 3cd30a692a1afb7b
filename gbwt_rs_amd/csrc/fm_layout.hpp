// fm_layout.hpp -- the FM-index over a text as kernels (fm_index.hip) and a host program (tests/cpp/fm_layout.cpp) both see it: block
// arithmetic, rank within a block and one backward step.  __host__ __device__, no HIP call, as sa_key.hpp and gfa_names.hpp.
//
// ROWS.  The suffix array of T[0, n) has n rows; backward search needs n + 1: row 0 is the empty suffix, whose BWT byte is T[n - 1], and
// row j + 1 is SA row j with BWT byte T[SA[j] - 1].  The row with SA[j] == 0 -- `primary`, here in row coordinates: j + 1 -- has no BWT byte:
// what a BWT file shows there is the call's sentinel, which may equal a byte of the text and must not count as one.  The index stores
// code 0 there, leaves the row out of every block count, and rank takes it out of the count within a block.
//
// CODES.  The sigma distinct bytes of T get the dense codes 0 .. sigma - 1 in byte order (code[b], FM_ABSENT for a byte T lacks); C[c] = text
// bytes smaller than the byte of code c.  The rows [1 + C[c], 1 + C[c] + occurrences of c) are the suffixes that start with c.
//
// BLOCKS.  Row i lies in block i / B; there are rows / B + 1 blocks, so that rank(c, rows) finds a block as well.
//   packed (sigma <= 8): a block is one 128-byte line -- eight u32 counts (occurrences of code c in the rows in front of the block), then
//                        B = 96 BWT codes, one per byte.  One rank reads one line.
//   plain  (sigma > 8):  B = 256 codes per block in `lines`, and counts[block * sigma + c] beside them: one rank reads the count's line and
//                        the at most two lines in front of row i in its block.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FM_HD __host__ __device__ inline
#else
#define FM_HD inline
#endif

namespace gbwt_hip {

constexpr uint32_t FM_PACKED_SIGMA = 8;       // the largest alphabet of the packed layout
constexpr uint32_t FM_LINE = 128;             // bytes of a packed block
constexpr uint32_t FM_PACKED_HEAD = 32;       // bytes of its counts
constexpr uint32_t FM_PACKED_BLOCK = 96;      // BWT codes behind them
constexpr uint32_t FM_PLAIN_BLOCK = 256;      // BWT codes of a plain block
constexpr uint16_t FM_ABSENT = 0xFFFF;        // code of a byte the text lacks

struct alignas(16) FmQuad { uint32_t w[4]; };  // sixteen BWT codes: one load

struct FmLayout {
    uint32_t sigma = 0, packed = 1;
    uint64_t rows = 1;                // n + 1
    uint64_t blocks = 1;              // rows / B + 1
    uint64_t primary = 0;             // the row without a BWT byte (SA row + 1); 0 for an empty text: then no row is left out
    const uint8_t *lines = nullptr;   // packed: blocks lines of 128 bytes; plain: blocks * 256 codes
    const uint32_t *counts = nullptr; // plain: blocks * sigma
};

FM_HD bool fm_is_packed(uint32_t sigma) { return sigma <= FM_PACKED_SIGMA; }
FM_HD uint32_t fm_block_rows(bool packed) { return packed ? FM_PACKED_BLOCK : FM_PLAIN_BLOCK; }
FM_HD uint64_t fm_blocks(uint64_t rows, bool packed) { return rows / fm_block_rows(packed) + 1; }
FM_HD uint64_t fm_block_of(uint64_t row, bool packed) { return packed ? row / FM_PACKED_BLOCK : row / FM_PLAIN_BLOCK; }
FM_HD uint32_t fm_block_bytes(bool packed) { return packed ? FM_LINE : FM_PLAIN_BLOCK; }   // of `lines` per block
// where the code of a row stands in `lines`
FM_HD uint64_t fm_code_at(uint64_t row, bool packed) {
    return packed ? (row / FM_PACKED_BLOCK) * FM_LINE + FM_PACKED_HEAD + row % FM_PACKED_BLOCK : row;
}

// 0x80 in every byte of x that equals the byte repeated in `pattern` (exact: no carry crosses a byte)
FM_HD uint32_t fm_equal_bytes(uint32_t x, uint32_t pattern) {
    x ^= pattern;
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | x | 0x7F7F7F7Fu);
}

FM_HD uint32_t fm_popcount(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<uint32_t>(__popc(x));
#else
    return static_cast<uint32_t>(__builtin_popcount(x));
#endif
}

// Occurrences of code c among the first k codes behind `codes` (16-byte aligned; k at most the codes of a block).  Whole quads are read:
// a block's storage is a whole number of them.
FM_HD uint32_t fm_count(const uint8_t *codes, uint32_t k, uint32_t c) {
    const FmQuad *q = reinterpret_cast<const FmQuad *>(codes);
    const uint32_t pattern = c * 0x01010101u;
    uint32_t found = 0;
    for (uint32_t at = 0; at < k; at += 16, q++) {
        const FmQuad v = *q;
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t first = at + 4 * j;
            if (first >= k) break;
            const uint32_t left = k - first;                                      // codes of this word that count (little-endian: the low bytes)
            const uint32_t mask = left >= 4 ? 0xFFFFFFFFu : (uint32_t(1) << (8 * left)) - 1;
            found += fm_popcount(fm_equal_bytes(v.w[j], pattern) & mask);
        }
    }
    return found;
}

// Occurrences of code c in the rows [first row of block b, first row + k) with the primary row left out: what a block contributes
FM_HD uint32_t fm_count_in_block(const FmLayout &L, uint64_t b, uint32_t k, uint32_t c) {
    const uint32_t B = fm_block_rows(L.packed != 0);
    const uint8_t *codes = L.packed ? L.lines + b * FM_LINE + FM_PACKED_HEAD : L.lines + b * FM_PLAIN_BLOCK;
    uint32_t found = fm_count(codes, k, c);
    const uint64_t first = b * B;
    if (c == 0 && L.primary != 0 && L.primary >= first && L.primary < first + k) found--;
    return found;
}

// rank(c, i): occurrences of code c in the rows [0, i), i <= rows
FM_HD uint64_t fm_rank(const FmLayout &L, uint32_t c, uint64_t i) {
    const uint32_t B = fm_block_rows(L.packed != 0);
    const uint64_t b = fm_block_of(i, L.packed != 0);
    const uint32_t k = static_cast<uint32_t>(i - b * B);
    const uint32_t before = L.packed ? reinterpret_cast<const uint32_t *>(L.lines + b * FM_LINE)[c] : L.counts[b * L.sigma + c];
    return uint64_t(before) + fm_count_in_block(L, b, k, c);
}

// One backward step of the range [lo, hi) of rows with code c
FM_HD void fm_step(const FmLayout &L, const uint32_t *C, uint32_t c, uint64_t &lo, uint64_t &hi) {
    lo = 1 + uint64_t(C[c]) + fm_rank(L, c, lo);
    hi = 1 + uint64_t(C[c]) + fm_rank(L, c, hi);
}

// The SA range [lo, hi) of a pattern, read backward until the range is empty: (0, 0) for a pattern that does not occur, (0, n) for the
// empty one.  Returns the backward steps taken.
FM_HD uint64_t fm_search(const FmLayout &L, const uint16_t *code, const uint32_t *C, const uint8_t *pattern, uint64_t len, uint64_t &out_lo, uint64_t &out_hi) {
    uint64_t lo = 0, hi = L.rows, steps = 0;
    for (uint64_t j = len; j > 0 && lo < hi; j--) {
        const uint16_t c = code[pattern[j - 1]];
        if (c == FM_ABSENT) { lo = hi = 0; break; }
        fm_step(L, C, c, lo, hi);
        steps++;
    }
    if (lo >= hi) { out_lo = out_hi = 0; return steps; }
    out_lo = lo == 0 ? 0 : lo - 1;                                                // SA coordinates: row 0 is no SA row
    out_hi = hi - 1;
    return steps;
}

}  // namespace gbwt_hip
