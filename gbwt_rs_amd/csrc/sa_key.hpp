// sa_key.hpp -- the sort keys of the suffix array builder (suffix_array.hip), shared with the host (tests/cpp/sa_key.cpp): one text for the
// kernels and for the program that checks the order without a GPU.
//
// The suffixes of T[0, n) are ordered as unsigned byte strings compared to the end of the text; a suffix that is a proper prefix of another
// is the smaller one.  The FIRST key of suffix i holds its first SA_KEY_BYTES = 7 bytes big-endian in the upper 56 bits and the number of
// bytes it really has there (1 .. 7) in the low byte; bytes past the end of the text are 0.  Two suffixes with different first keys are
// ordered by them: either a byte differs, or the bytes agree -- the missing ones being 0 -- and the one with fewer bytes is a proper prefix
// of the other (or has only 0 bytes where the other has more of the text), and fewer sorts first.  Equal first keys mean seven equal bytes
// that both suffixes have.
//
// The key of a ROUND is (rank of the group, rank of the suffix h positions on) in 2 * sa_rank_bits(n) bits: ranks start at 1, the second
// rank of a suffix that ends within h positions is 0 -- it is a proper prefix of every other suffix of its group.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GBWT_SA_HD __host__ __device__ inline
#else
#define GBWT_SA_HD inline
#endif

namespace gbwt_hip {

constexpr uint32_t SA_KEY_BYTES = 7;

// The first key from the eight bytes at a suffix as two little-endian words (lo = bytes 0 .. 3, hi = bytes 4 .. 7, whatever lies behind the
// text in them) and the bytes the suffix has, at most SA_KEY_BYTES of them: 1 <= valid <= 7
GBWT_SA_HD uint64_t sa_first_key(uint32_t lo, uint32_t hi, uint32_t valid) {
    const uint32_t a = __builtin_bswap32(lo), b = __builtin_bswap32(hi);
    const uint64_t bytes = (static_cast<uint64_t>(a) << 32) | b;
    return (bytes & (~uint64_t(0) << (64 - 8 * valid))) | valid;
}

// The same from the text itself, byte by byte (the host's form; the pack kernel reads words)
GBWT_SA_HD uint64_t sa_first_key_at(const uint8_t *text, uint64_t n, uint64_t i) {
    const uint64_t left = n - i;
    const uint32_t valid = left < SA_KEY_BYTES ? static_cast<uint32_t>(left) : SA_KEY_BYTES;
    uint64_t key = 0;
    for (uint32_t k = 0; k < valid; k++) key |= static_cast<uint64_t>(text[i + k]) << (56 - 8 * k);
    return key | valid;
}

// Bits of a rank: ranks are 0 .. n
GBWT_SA_HD uint32_t sa_rank_bits(uint64_t n) {
    uint32_t bits = 1;
    while (bits < 64 && (n >> bits) != 0) bits++;
    return bits;
}

GBWT_SA_HD uint64_t sa_round_key(uint32_t group, uint32_t second, uint32_t rank_bits) { return (static_cast<uint64_t>(group) << rank_bits) | second; }

// The second rank of suffix p in a round of step h: that of suffix p + h, 0 past the end
GBWT_SA_HD uint32_t sa_second_rank(const uint32_t *rank, uint64_t n, uint64_t p, uint64_t h) { return p + h < n ? rank[p + h] : 0u; }

}  // namespace gbwt_hip
