// gfa_names.cpp -- the name table of a translated construction from GFA (csrc/gfa_names.hpp) on the host, as a program of its own for
// ASan + UBSan: the table is built the way gfa_parse.hip builds it (hash, stable sort by hash, one bisection per bucket), once with the
// real hash and once with a constant one, which puts every name into one bucket and one run of equal hashes.
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "gfa_names.hpp"

using namespace gbwt_hip;

namespace {

struct ConstantHash {
    uint64_t operator()(const uint8_t *, uint32_t) const { return 0x8000000000000001ull; }
};

int failures = 0;
void expect(bool ok, const std::string &what) {
    if (!ok) { std::printf("FAIL %s\n", what.c_str()); failures++; }
}

struct Table {
    std::vector<uint8_t> text;
    std::vector<uint64_t> name_lo, hash;
    std::vector<uint32_t> name_len, rank, bucket;
    GfaNameTable view{};
};

template <class Hash>
void build(const std::vector<std::string> &names, Hash hash_of, Table &t) {
    const size_t n = names.size();
    for (const std::string &s : names) {
        t.text.push_back('\t');
        t.name_lo.push_back(t.text.size());
        t.name_len.push_back(static_cast<uint32_t>(s.size()));
        t.text.insert(t.text.end(), s.begin(), s.end());
    }
    t.text.push_back('\n');
    std::vector<uint64_t> by_rank(n);
    for (size_t k = 0; k < n; k++) by_rank[k] = hash_of(t.text.data() + t.name_lo[k], t.name_len[k]);
    t.rank.resize(n);
    std::iota(t.rank.begin(), t.rank.end(), 0u);
    std::stable_sort(t.rank.begin(), t.rank.end(), [&](uint32_t a, uint32_t b) { return by_rank[a] < by_rank[b]; });
    for (uint32_t k : t.rank) t.hash.push_back(by_rank[k]);
    const uint32_t bits = gfa_bucket_bits(n);
    const uint64_t buckets = uint64_t(1) << bits;
    t.bucket.resize(buckets + 1);
    for (uint64_t b = 0; b <= buckets; b++)
        t.bucket[b] = b == buckets ? static_cast<uint32_t>(n) : static_cast<uint32_t>(std::lower_bound(t.hash.begin(), t.hash.end(), gfa_bucket_floor(b, bits)) - t.hash.begin());
    t.view = GfaNameTable{t.text.data(), t.name_lo.data(), t.name_len.data(), t.hash.data(), t.rank.data(), t.bucket.data(), bits, static_cast<uint32_t>(n)};
}

template <class Hash>
uint32_t find(const Table &t, const std::string &s, Hash hash_of) {
    const std::vector<uint8_t> copy(s.begin(), s.end());       // (its own allocation: a read past the name is ASan's to find)
    return gfa_lookup_name(t.view, copy.data(), static_cast<uint32_t>(copy.size()), hash_of);
}

template <class Hash>
void run(const char *label, Hash hash_of) {
    const std::string long_a(255, 'a'), long_b = std::string(254, 'a') + "b";
    // ranks:                             0    1     2      3     4    5       6       7     8     9 (= 1)  10    11 (= 4)
    const std::vector<std::string> names{"s", "s1", "s11", "11", "1", long_a, long_b, "s+", "-s", "s1",    "+",  "1"};
    Table t;
    build(names, hash_of, t);
    const std::string at = std::string(label) + ": ";
    for (size_t k = 0; k < names.size(); k++) {
        const size_t first = static_cast<size_t>(std::find(names.begin(), names.end(), names[k]) - names.begin());
        expect(find(t, names[k], hash_of) == first, at + "lookup of rank " + std::to_string(k));
    }
    for (const std::string &absent : {std::string("s111"), std::string("S"), std::string(""), std::string(254, 'a'), std::string(256, 'a'), std::string("s-"), std::string("2")})
        expect(find(t, absent, hash_of) == GFA_NO_SEGMENT, at + "absent name of " + std::to_string(absent.size()) + " bytes");
    std::vector<uint32_t> repeats;
    for (uint32_t i = 0; i < names.size(); i++)
        if (gfa_name_repeats(t.view, i)) repeats.push_back(t.rank[i]);
    std::sort(repeats.begin(), repeats.end());
    expect(repeats == std::vector<uint32_t>{9, 11}, at + "the later S-lines of a name");
    uint32_t longest = 0;
    for (size_t b = 0; b + 1 < t.bucket.size(); b++) {
        expect(t.bucket[b] <= t.bucket[b + 1], at + "bucket bounds ascend");
        longest = std::max(longest, t.bucket[b + 1] - t.bucket[b]);
    }
    expect(t.bucket.front() == 0 && t.bucket.back() == names.size(), at + "the buckets cover the table");
    std::printf("%s buckets %zu longest %u bits %u\n", label, t.bucket.size() - 1, longest, t.view.bits);

    Table one;                                                 // one segment: no bits, one bucket
    build(std::vector<std::string>{"only"}, hash_of, one);
    expect(one.view.bits == 0 && find(one, "only", hash_of) == 0 && find(one, "onl", hash_of) == GFA_NO_SEGMENT, at + "a table of one name");
    Table none;
    build(std::vector<std::string>{}, hash_of, none);
    expect(find(none, "x", hash_of) == GFA_NO_SEGMENT, at + "an empty table");
}

}  // namespace

int main() {
    run("real", GfaNameHash());
    run("constant", ConstantHash());
    expect(gfa_bucket_bits(1) == 0 && gfa_bucket_bits(2) == 1 && gfa_bucket_bits(3) == 2 && gfa_bucket_bits(4) == 2 && gfa_bucket_bits(5) == 3 &&
           gfa_bucket_bits(uint64_t(1) << 40) == 31, "bucket bits");
    expect(gfa_bucket_of(~uint64_t(0), 3) == 7 && gfa_bucket_of(~uint64_t(0), 0) == 0 && gfa_bucket_floor(7, 3) == 0xE000000000000000ull, "bucket of a hash");
    std::printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
