// fm_align.hpp -- the alignments of chains (include/gbwt_hip.h, "Alignments of chains") as kernels (fm_align.hip) and a host
// program (tests/cpp/fm_align.cpp) both see them: the band of a chain, which cells of it exist, the rule of a cell and its direction, how
// the directions of a row are packed, the walk back through them and the packing of a CIGAR.  __host__ __device__, no HIP call, as
// fm_chains.hpp.
//
// THE BAND.  A member (y, x, w) of a chain lies on the diagonal d = y - x, signed.  d0 = min d - band, d1 = max d + band, W = d1 - d0 + 1:
// the cells of row i are the diagonals k = 0 .. W - 1, cell (i, k) standing at text position j = i + d0 + k.
// EXISTENCE.  Cell (i, k) exists when lo <= j <= hi, the bounds of the segment: in a row the cells that exist are one stretch of k.
// THE CELL.  Row 0 is 0 where it exists.  Below it A(i, k) = min(H(i - 1, k) + (P[i - 1] != T[j - 1]), H(i - 1, k + 1) + 1) over the
// neighbours that exist and are reachable, the diagonal first on a tie; H(i, k) = min(A(i, k), H(i, k - 1) + 1), the deletion only where
// it is strictly smaller.  FM_ALIGN_INF stands for unreachable; a reachable H is at most L (see fm_align_plan.hpp), so +1 never wraps.
// DIRECTIONS.  2 bits per cell, 16 cells to a u32: cell k of a row is bit k % 16 (low bit of the direction) and bit 16 + k % 16 (high
// bit) of word k / 16 -- the halves of two wave ballots, so no lane shifts a direction to its place.
#pragma once

#include <cstdint>

#include "../../include/gbwt_hip.h"
#include "fm_layout.hpp"

namespace gbwt_hip {

constexpr uint32_t FM_ALIGN_MAX_WIDTH = 1024;                  // the widest band: 16 diagonals per lane of a wave
constexpr uint32_t FM_ALIGN_DEFAULT_BAND = 16, FM_ALIGN_DEFAULT_WIDTH = 256;
constexpr uint32_t FM_ALIGN_MAX_READ = (1u << 28) - 1;          // the length of a run fits in the 28 bits of a CIGAR entry
constexpr uint64_t FM_ALIGN_TILE_BYTES = 8192;                 // the directions of an alignment that k_align_dp keeps in LDS, per wave
constexpr uint64_t FM_ALIGN_TEXT_TILE = 1536;                  // the text window of an alignment that k_align_dp stages in LDS, per wave
constexpr uint32_t FM_ALIGN_INF = 0xFFFFFFFFu;                // an unreachable cell; the edit_distance of GBWT_HIP_ALIGN_NONE
constexpr uint32_t FM_ALIGN_DIAGONAL = 0, FM_ALIGN_INSERTION = 1, FM_ALIGN_DELETION = 2;
constexpr uint32_t FM_CIGAR_I = 1, FM_CIGAR_D = 2, FM_CIGAR_EQ = 7, FM_CIGAR_X = 8;      // BAM's codes

// The diagonal of a member: y a text position (it may exceed 2^31), x a read position
FM_HD int64_t fm_align_diagonal(uint64_t y, uint32_t x) { return static_cast<int64_t>(y) - static_cast<int64_t>(x); }

// d0 and W of the diagonals [dmin, dmax] widened by `band`.  W is u64: the members of a chain may lie 2^32 apart
FM_HD int64_t fm_align_d0(int64_t dmin, uint32_t band) { return dmin - static_cast<int64_t>(band); }
FM_HD uint64_t fm_align_width(int64_t dmin, int64_t dmax, uint32_t band) { return static_cast<uint64_t>(dmax - dmin) + 2 * static_cast<uint64_t>(band) + 1; }

// max_width as the arithmetic takes it
FM_HD uint32_t fm_align_max_width(uint32_t max_width) { return max_width == 0 ? FM_ALIGN_DEFAULT_WIDTH : max_width; }

// The cells of row i that exist: k in [first, last], empty where first > last.  lo, hi: the first text position of the segment and the
// one behind its last base (cell j = hi exists: an alignment may end there)
FM_HD void fm_align_row_range(int64_t d0, uint32_t W, uint64_t lo, uint64_t hi, uint32_t i, int32_t &first, int32_t &last) {
    const int64_t base = d0 + static_cast<int64_t>(i);                          // j of k == 0
    const int64_t a = static_cast<int64_t>(lo) - base, b = static_cast<int64_t>(hi) - base;
    first = a <= 0 ? 0 : a >= static_cast<int64_t>(W) ? static_cast<int32_t>(W) : static_cast<int32_t>(a);
    last = b < 0 ? -1 : b >= static_cast<int64_t>(W) ? static_cast<int32_t>(W) - 1 : static_cast<int32_t>(b);
}

// A(i, k) and its direction from the two neighbours of the row above (FM_ALIGN_INF: none, or unreachable)
FM_HD uint32_t fm_align_cell(uint32_t diagonal, bool mismatch, uint32_t insertion, uint32_t &direction) {
    const uint32_t by_diagonal = diagonal == FM_ALIGN_INF ? FM_ALIGN_INF : diagonal + (mismatch ? 1u : 0u);
    const uint32_t by_insertion = insertion == FM_ALIGN_INF ? FM_ALIGN_INF : insertion + 1;
    direction = by_insertion < by_diagonal ? FM_ALIGN_INSERTION : FM_ALIGN_DIAGONAL;
    return by_insertion < by_diagonal ? by_insertion : by_diagonal;
}

// H(i, k) from A(i, k) and H(i, k - 1) (FM_ALIGN_INF: none): the deletion only where it is strictly smaller
FM_HD uint32_t fm_align_delete(uint32_t a, uint32_t left, uint32_t &direction) {
    if (left == FM_ALIGN_INF || left + 1 >= a) return a;
    direction = FM_ALIGN_DELETION;
    return left + 1;
}

// The deletion chain of a row as a prefix minimum: H(k) = min over k' <= k of (A(k') + k - k'), so H(k) + (BIAS - k) is the prefix minimum
// of A(k') + (BIAS - k').  FM_ALIGN_INF stays what it is
FM_HD uint32_t fm_align_skew(uint32_t a, uint32_t k) { return a == FM_ALIGN_INF ? FM_ALIGN_INF : a + (FM_ALIGN_MAX_WIDTH - k); }
FM_HD uint32_t fm_align_unskew(uint32_t v, uint32_t k) { return v == FM_ALIGN_INF ? FM_ALIGN_INF : v - (FM_ALIGN_MAX_WIDTH - k); }

// The key one reduction over row L picks the result with: the smallest H, then the smallest k
FM_HD uint64_t fm_align_end_key(uint32_t h, uint32_t k) { return (static_cast<uint64_t>(h) << 32) | k; }

// The directions of a row: words, bytes of an alignment, and cell k of a row
FM_HD uint32_t fm_align_row_words(uint32_t W) { return (W + 15) / 16; }
FM_HD uint64_t fm_align_direction_bytes(uint32_t L, uint32_t W) { return static_cast<uint64_t>(L) * fm_align_row_words(W) * sizeof(uint32_t); }
FM_HD uint32_t fm_align_direction_word(uint64_t low_bits, uint64_t high_bits, uint32_t word_in_chunk) {      // the ballots of a chunk of 64 cells
    return static_cast<uint32_t>((low_bits >> (16 * word_in_chunk)) & 0xFFFFu) | (static_cast<uint32_t>((high_bits >> (16 * word_in_chunk)) & 0xFFFFu) << 16);
}
FM_HD uint32_t fm_align_direction_at(uint32_t word, uint32_t k) { return ((word >> (k % 16)) & 1u) | (((word >> (16 + k % 16)) & 1u) << 1); }

// Do the directions of an alignment fit the tile?  And the entries its CIGAR may have (fm_align_plan.hpp says why)
FM_HD bool fm_align_in_tile(uint64_t L, uint64_t W) { return L * ((W + 15) / 16) * sizeof(uint32_t) <= FM_ALIGN_TILE_BYTES; }
FM_HD uint64_t fm_align_cigar_bound(uint64_t L) { return 2 * L; }

FM_HD uint32_t fm_cigar_entry(uint32_t length, uint32_t op) { return (length << 4) | op; }

// The walk back from (L, k_end) to row 0 through the directions (row i >= 1 at directions + (i - 1) * fm_align_row_words(W)).  The runs
// are written backward: the last entry of the CIGAR at entries[capacity - 1], and the first at entries[capacity - returned count].
// read(i): P[i]; text(j): T[j].  Returns the entries; k_start: the diagonal at row 0.
template <class Directions, class Read, class Text>
FM_HD uint32_t fm_align_trace(uint32_t L, uint32_t W, int64_t d0, uint32_t k_end, Directions directions, Read read, Text text, uint32_t *entries, uint32_t capacity, uint32_t &k_start) {
    const uint32_t words = fm_align_row_words(W);
    uint32_t i = L, k = k_end, count = 0, run = 0, run_op = 0;
    while (i > 0) {
        const uint32_t direction = fm_align_direction_at(directions[static_cast<uint64_t>(i - 1) * words + k / 16], k);
        uint32_t op;
        if (direction == FM_ALIGN_DIAGONAL) {
            const uint64_t j = static_cast<uint64_t>(d0 + static_cast<int64_t>(i) + static_cast<int64_t>(k));
            op = read(i - 1) == text(j - 1) ? FM_CIGAR_EQ : FM_CIGAR_X;
            i--;
        } else if (direction == FM_ALIGN_INSERTION) {
            if (k + 1 >= W) break;                       // (never: an insertion comes from a cell of the band)
            op = FM_CIGAR_I;
            i--;
            k++;
        } else {
            if (k == 0) break;
            op = FM_CIGAR_D;
            k--;
        }
        if (run != 0 && op != run_op) {
            if (count + 1 >= capacity) break;            // (never with directions the rule wrote: the bound holds)
            entries[capacity - ++count] = fm_cigar_entry(run, run_op);
            run = 0;
        }
        run_op = op;
        run++;
    }
    if (run != 0) entries[capacity - ++count] = fm_cigar_entry(run, run_op);
    k_start = k;
    return count;
}

}  // namespace gbwt_hip
