// sa_key.cpp -- csrc/sa_key.hpp on the host (tests/test_sa_cpu.py builds it with ASan + UBSan): the order of the first keys against the
// order of the suffixes themselves, the word form of the key against the byte form, and the keys of a round.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sa_key.hpp"

using namespace gbwt_hip;

static int failures = 0;
static void expect(bool ok, const char *name) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
    if (!ok) failures++;
}

// suffix a of text < suffix b: unsigned bytes to the end of the text, a proper prefix first
static bool suffix_less(const std::string &t, size_t a, size_t b) {
    const size_t la = t.size() - a, lb = t.size() - b, common = std::min(la, lb);
    const int c = std::memcmp(t.data() + a, t.data() + b, common);
    return c != 0 ? c < 0 : la < lb;
}

// The key of suffix i as the pack kernel cuts it: two little-endian words from the eight bytes at i, whatever lies behind the text in them
static uint64_t key_from_words(const std::string &t, size_t i, uint8_t junk) {
    uint8_t window[8];
    for (size_t k = 0; k < 8; k++) window[k] = i + k < t.size() ? static_cast<uint8_t>(t[i + k]) : junk;
    uint32_t lo, hi;
    std::memcpy(&lo, window, 4);
    std::memcpy(&hi, window + 4, 4);
    const size_t rest = t.size() - i;
    return sa_first_key(lo, hi, rest < SA_KEY_BYTES ? static_cast<uint32_t>(rest) : SA_KEY_BYTES);
}

// Over every pair of suffixes of the text: different keys order as the suffixes do, equal keys mean seven bytes that both have and that agree
static bool keys_agree_with_suffixes(const std::string &t) {
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(t.data());
    for (size_t a = 0; a < t.size(); a++) {
        const uint64_t ka = sa_first_key_at(bytes, t.size(), a);
        if (ka != key_from_words(t, a, 0) || ka != key_from_words(t, a, 0xFF)) return false;
        for (size_t b = 0; b < t.size(); b++) {
            if (a == b) continue;
            const uint64_t kb = sa_first_key_at(bytes, t.size(), b);
            if (ka != kb) { if ((ka < kb) != suffix_less(t, a, b)) return false; continue; }
            if (t.size() - a < SA_KEY_BYTES || t.size() - b < SA_KEY_BYTES || std::memcmp(bytes + a, bytes + b, SA_KEY_BYTES) != 0) return false;
        }
    }
    return true;
}

int main() {
    // every byte string of length <= 3 over {0, 1, 255}, alone, and as the tail of a text of two of them with seven equal bytes in between
    const char alphabet[3] = {'\0', '\1', '\xFF'};
    std::vector<std::string> strings{""};
    for (size_t first = 0, len = 1; len <= 3; len++) {
        const size_t end = strings.size();
        for (size_t k = first; k < end; k++)
            for (char c : alphabet) strings.push_back(strings[k] + c);
        first = end;
    }
    expect(strings.size() == 1 + 3 + 9 + 27, "strings_of_length_0_to_3");
    bool alone = true, pairs = true;
    for (const std::string &s : strings) alone = alone && keys_agree_with_suffixes(s);
    expect(alone, "short_strings_alone");
    // the keys of two strings against each other: as suffixes they would be compared to their ends
    for (const std::string &s : strings)
        for (const std::string &u : strings) {
            if (s.empty() || u.empty() || s == u) continue;
            const uint64_t ks = sa_first_key_at(reinterpret_cast<const uint8_t *>(s.data()), s.size(), 0), ku = sa_first_key_at(reinterpret_cast<const uint8_t *>(u.data()), u.size(), 0);
            const size_t common = std::min(s.size(), u.size());
            const int c = std::memcmp(s.data(), u.data(), common);
            const bool less = c != 0 ? c < 0 : s.size() < u.size();
            pairs = pairs && ks != ku && (ks < ku) == less;
        }
    expect(pairs, "short_strings_against_each_other");
    // the tail of a text: suffixes shorter than the key, with zeros and with the bytes of longer suffixes in front of them
    expect(keys_agree_with_suffixes(std::string("ACGTACGTACGTAC\0\0A\0\0", 19)), "tail_with_zeros");
    expect(keys_agree_with_suffixes(std::string("AAAAAAAAAAAAAAAA")), "tail_of_a_run");
    expect(keys_agree_with_suffixes(std::string("\0\0\0\0\0\0\0\0\0\0", 10)), "tail_of_zeros");
    expect(keys_agree_with_suffixes(std::string("\xFF\xFF\xFF\xFF\xFF\xFF\xFF\xFF\xFF")), "tail_of_255");
    expect(keys_agree_with_suffixes(std::string("ABABABABABABABAB\0", 17)), "periodic_with_endmarker");
    // the low byte is the number of bytes, the upper 56 bits the bytes
    const uint8_t text[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
    expect(sa_first_key_at(text, 9, 0) == 0x0102030405060707ull, "key_layout_full");
    expect(sa_first_key_at(text, 9, 6) == 0x0708090000000003ull, "key_layout_tail");
    // widths and the keys of a round
    expect(sa_rank_bits(1) == 1 && sa_rank_bits(2) == 2 && sa_rank_bits(3) == 2 && sa_rank_bits(4) == 3 && sa_rank_bits(0xFFFFFFFEull) == 32, "rank_bits");
    expect(sa_round_key(5, 0, 3) == 40 && sa_round_key(5, 7, 3) == 47 && sa_round_key(0xFFFFFFFEu, 0xFFFFFFFEu, 32) == 0xFFFFFFFEFFFFFFFEull, "round_key");
    expect(sa_round_key(2, 7, 3) < sa_round_key(3, 0, 3), "round_key_group_first");
    const uint32_t rank[4] = {4, 3, 2, 1};
    expect(sa_second_rank(rank, 4, 1, 2) == 1 && sa_second_rank(rank, 4, 2, 2) == 0 && sa_second_rank(rank, 4, 3, 0xFFFFFFFFFFull) == 0, "second_rank");
    std::printf("%s\n", failures == 0 ? "done" : "failed");
    return failures == 0 ? 0 : 1;
}
