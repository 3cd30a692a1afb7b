// gfa_names.hpp -- the name table of a translated construction from GFA: the hash of a segment name and the lookup of a
// name among the S-lines.  The same code runs in the kernels of gfa_parse.hip and on the host (tests/cpp/gfa_names.cpp builds it with
// the sanitizers, with the real hash and with a constant one): the lookup is templated on the hash.
//
// The table: the S-lines ranked in file order; (hash, rank) sorted by hash (stably: the ranks of one hash ascend); bucket[b] = the first
// sorted entry whose hash has the top `bits` bits >= b, for b = 0 .. 2^bits (the last entry: the number of segments).  A lookup reads
// its bucket's two bounds, walks the entries of the bucket -- about one with bits = ceil(log2(segments)) -- and compares the bytes of
// those with its hash.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GFA_NAMES_HD __host__ __device__ __forceinline__
#else
#define GFA_NAMES_HD inline
#endif

namespace gbwt_hip {

// A name is 1 .. 255 bytes without tab or newline
constexpr uint32_t GFA_MAX_NAME = 255;

// FNV-1a over the bytes, then the finalizer of splitmix64: the buckets take the TOP bits, which plain FNV mixes least
struct GfaNameHash {
    GFA_NAMES_HD uint64_t operator()(const uint8_t *p, uint32_t len) const {
        uint64_t h = 0xCBF29CE484222325ull;
        for (uint32_t i = 0; i < len; i++) h = (h ^ p[i]) * 0x100000001B3ull;
        h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
        h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
        return h ^ (h >> 31);
    }
};

// ceil(log2(n)) for n >= 1, at most 31: the bits of a bucket index
GFA_NAMES_HD uint32_t gfa_bucket_bits(uint64_t n) {
    uint32_t bits = 0;
    while (bits < 31 && (uint64_t(1) << bits) < n) bits++;
    return bits;
}

GFA_NAMES_HD uint64_t gfa_bucket_of(uint64_t hash, uint32_t bits) { return bits ? hash >> (64 - bits) : 0; }

// The smallest hash of bucket b (b <= 2^bits; the bound behind the last bucket is never asked for)
GFA_NAMES_HD uint64_t gfa_bucket_floor(uint64_t b, uint32_t bits) { return bits ? b << (64 - bits) : 0; }

struct GfaNameTable {
    const uint8_t *text;         // the GFA text
    const uint64_t *name_lo;     // [segments] by rank: where the name starts
    const uint32_t *name_len;    // [segments] by rank
    const uint64_t *hash;        // [segments] sorted
    const uint32_t *rank;        // [segments] the rank of the sorted entry
    const uint32_t *bucket;      // [2^bits + 1]
    uint32_t bits;
    uint32_t segments;
};

GFA_NAMES_HD bool gfa_same_bytes(const uint8_t *a, const uint8_t *b, uint32_t len) {
    for (uint32_t i = 0; i < len; i++)
        if (a[i] != b[i]) return false;
    return true;
}

constexpr uint32_t GFA_NO_SEGMENT = 0xFFFFFFFFu;

// The rank of the S-line named p[0 .. len), the FIRST in file order if several have the name; GFA_NO_SEGMENT if none has
template <class Hash>
GFA_NAMES_HD uint32_t gfa_lookup_name(const GfaNameTable &t, const uint8_t *p, uint32_t len, Hash hash_of) {
    if (len == 0 || len > GFA_MAX_NAME || t.segments == 0) return GFA_NO_SEGMENT;
    const uint64_t h = hash_of(p, len), b = gfa_bucket_of(h, t.bits);
    for (uint32_t i = t.bucket[b], end = t.bucket[b + 1]; i < end; i++) {
        if (t.hash[i] != h) continue;
        const uint32_t k = t.rank[i];
        if (t.name_len[k] == len && gfa_same_bytes(t.text + t.name_lo[k], p, len)) return k;
    }
    return GFA_NO_SEGMENT;
}

// Whether sorted entry i names the same segment as an earlier entry of its run of equal hashes (i.e. its S-line is a later duplicate)
GFA_NAMES_HD bool gfa_name_repeats(const GfaNameTable &t, uint32_t i) {
    const uint32_t k = t.rank[i];
    for (uint32_t j = i; j > 0 && t.hash[j - 1] == t.hash[i]; j--) {
        const uint32_t e = t.rank[j - 1];
        if (t.name_len[e] == t.name_len[k] && gfa_same_bytes(t.text + t.name_lo[e], t.text + t.name_lo[k], t.name_len[k])) return true;
    }
    return false;
}

}  // namespace gbwt_hip
