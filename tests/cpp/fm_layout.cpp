// fm_layout.cpp -- csrc/fm_layout.hpp on the host (tests/test_fm_cpu.py builds it with ASan + UBSan): the blocks are filled here the way
// the kernels of fm_index.hip fill them -- codes through fm_code_at, block counts through fm_count_in_block, their sums in front of every
// block -- and rank, single steps and whole backward searches are compared with counts made naively from the text and its sorted suffixes.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "fm_layout.hpp"

using namespace gbwt_hip;

static int failures = 0;
static void expect(bool ok, const std::string &name) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name.c_str());
    if (!ok) failures++;
}

using Text = std::vector<uint8_t>;

// suffixes as unsigned byte strings compared to the end of the text, a proper prefix first
static std::vector<uint64_t> suffix_array(const Text &t) {
    std::vector<uint64_t> sa(t.size());
    for (size_t i = 0; i < sa.size(); i++) sa[i] = i;
    std::sort(sa.begin(), sa.end(), [&](uint64_t a, uint64_t b) {
        const size_t la = t.size() - a, lb = t.size() - b;
        const int c = std::memcmp(t.data() + a, t.data() + b, std::min(la, lb));
        return c != 0 ? c < 0 : la < lb;
    });
    return sa;
}

struct HostIndex {
    FmLayout L;
    std::vector<FmQuad> lines;        // 16-byte aligned, whole blocks
    std::vector<uint32_t> counts;
    uint16_t code[256];
    uint32_t C[256];
    std::vector<uint64_t> sa;
};

static void build(const Text &t, HostIndex &h) {
    const uint64_t n = t.size();
    uint64_t hist[256] = {};
    for (uint8_t b : t) hist[b]++;
    uint32_t sigma = 0;
    uint64_t smaller = 0;
    for (int b = 0; b < 256; b++) {
        h.code[b] = FM_ABSENT;
        h.C[b] = 0;
        if (!hist[b]) continue;
        h.code[b] = static_cast<uint16_t>(sigma);
        h.C[sigma++] = static_cast<uint32_t>(smaller);
        smaller += hist[b];
    }
    const bool packed = fm_is_packed(sigma);
    h.sa = suffix_array(t);
    FmLayout &L = h.L;
    L.sigma = sigma; L.packed = packed ? 1 : 0; L.rows = n + 1; L.blocks = fm_blocks(n + 1, packed); L.primary = 0;
    h.lines.assign(L.blocks * fm_block_bytes(packed) / sizeof(FmQuad), FmQuad{});
    uint8_t *bytes = reinterpret_cast<uint8_t *>(h.lines.data());
    L.lines = bytes;
    for (uint64_t row = 0; row <= n && n; row++) {
        uint8_t c = 0;
        if (row == 0) c = static_cast<uint8_t>(h.code[t[n - 1]]);
        else if (h.sa[row - 1] == 0) L.primary = row;
        else c = static_cast<uint8_t>(h.code[t[h.sa[row - 1] - 1]]);
        bytes[fm_code_at(row, packed)] = c;
    }
    const uint32_t B = fm_block_rows(packed);
    std::vector<uint32_t> in_block(uint64_t(sigma) * L.blocks, 0);
    for (uint64_t b = 0; b < L.blocks && n; b++) {
        const uint64_t first = b * B;
        const uint32_t k = first >= L.rows ? 0 : static_cast<uint32_t>(std::min<uint64_t>(B, L.rows - first));
        for (uint32_t c = 0; c < sigma; c++) in_block[c * L.blocks + b] = fm_count_in_block(L, b, k, c);
    }
    h.counts.assign(packed ? 0 : L.blocks * sigma, 0);
    for (uint32_t c = 0; c < sigma; c++) {
        uint32_t before = 0;
        for (uint64_t b = 0; b < L.blocks; b++) {
            if (packed) reinterpret_cast<uint32_t *>(bytes + b * FM_LINE)[c] = before;
            else h.counts[b * sigma + c] = before;
            before += in_block[c * L.blocks + b];
        }
    }
    L.counts = h.counts.data();
}

// the SA range of a pattern by looking at every suffix
static void naive_range(const Text &t, const std::vector<uint64_t> &sa, const Text &p, uint64_t &lo, uint64_t &hi) {
    lo = hi = 0;
    bool found = false;
    for (uint64_t j = 0; j < sa.size(); j++) {
        const bool starts = t.size() - sa[j] >= p.size() && (p.empty() || std::memcmp(t.data() + sa[j], p.data(), p.size()) == 0);
        if (starts && !found) { lo = j; found = true; }
        if (starts) hi = j + 1;
    }
}

// Everything about one text: rank against the BWT written out with `sentinel` at the primary row, and searches against naive_range
static bool check_text(const Text &t, uint8_t sentinel, std::mt19937 &rng) {
    HostIndex h;
    build(t, h);
    const uint64_t n = t.size();
    bool ok = true;
    // the BWT of the n + 1 rows; the sentinel at the primary row is a byte like any other here, and must not be counted
    std::vector<uint8_t> bwt(n + 1, 0);
    for (uint64_t row = 0; row <= n && n; row++) bwt[row] = row == 0 ? t[n - 1] : (h.sa[row - 1] == 0 ? sentinel : t[h.sa[row - 1] - 1]);
    for (int b = 0; b < 256 && n; b++) {
        if (h.code[b] == FM_ABSENT) continue;
        uint64_t seen = 0;
        for (uint64_t i = 0; i <= n + 1; i++) {
            ok = ok && fm_rank(h.L, h.code[b], i) == seen;
            if (i <= n && bwt[i] == b && i != h.L.primary) seen++;
        }
    }
    // patterns: empty, every byte value, substrings of several lengths, the whole text, the text and one byte, a miss inside
    std::vector<Text> patterns{Text{}, t};
    for (int b = 0; b < 256; b++) patterns.push_back(Text{static_cast<uint8_t>(b)});
    for (uint32_t len : {1u, 2u, 3u, 9u, 40u})
        for (int k = 0; k < 40 && n >= len; k++) {
            const uint64_t at = rng() % (n - len + 1);
            patterns.emplace_back(t.begin() + at, t.begin() + at + len);
            Text miss = patterns.back();
            miss[rng() % len] = t[rng() % n];
            patterns.push_back(miss);
        }
    for (uint32_t len = 1; len <= 5 && len <= n; len++) { patterns.emplace_back(t.begin(), t.begin() + len); patterns.emplace_back(t.end() - len, t.end()); }
    Text longer = t;
    longer.push_back(n ? t[0] : 65);
    patterns.push_back(longer);
    for (const Text &p : patterns) {
        uint64_t lo = 0, hi = 0, want_lo = 0, want_hi = 0;
        const uint64_t steps = fm_search(h.L, h.code, h.C, p.data(), p.size(), lo, hi);
        naive_range(t, h.sa, p, want_lo, want_hi);
        if (p.empty()) { want_lo = 0; want_hi = n; }
        ok = ok && lo == want_lo && hi == want_hi && steps <= p.size();
    }
    return ok;
}

static Text random_text(uint64_t n, uint32_t sigma, std::mt19937 &rng) {
    static const uint8_t six[6] = {0, 'A', 'C', 'G', 'N', 'T'};
    Text t(n);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t v = i < sigma ? static_cast<uint32_t>(i) : rng() % sigma;       // every symbol, where the length allows
        t[i] = sigma == 1 ? 'A' : sigma == 6 ? six[v] : static_cast<uint8_t>(v);
    }
    std::shuffle(t.begin(), t.end(), rng);
    return t;
}

int main() {
    std::mt19937 rng(19);
    // the SWAR count against a loop
    {
        alignas(16) uint8_t codes[256];
        for (int i = 0; i < 256; i++) codes[i] = static_cast<uint8_t>(rng() % 5 == 0 ? 255 : rng() % 3);
        bool ok = true;
        for (uint32_t c : {0u, 1u, 2u, 255u})
            for (uint32_t k = 0; k <= 256; k++) {
                uint32_t want = 0;
                for (uint32_t i = 0; i < k; i++) want += codes[i] == c;
                ok = ok && fm_count(codes, k, c) == want;
            }
        expect(ok, "count_prefixes_0_to_256");
    }
    expect(fm_blocks(96, true) == 2 && fm_blocks(95, true) == 1 && fm_blocks(256, false) == 2 && fm_code_at(96, true) == 128 + 32 && fm_code_at(95, true) == 32 + 95 &&
               fm_code_at(300, false) == 300 && fm_is_packed(8) && !fm_is_packed(9),
           "block_arithmetic");
    // an empty text: one row, every pattern but the empty one misses
    {
        HostIndex h;
        build(Text{}, h);
        uint64_t lo = 7, hi = 7;
        const Text a{'A'};
        fm_search(h.L, h.code, h.C, a.data(), 1, lo, hi);
        bool ok = lo == 0 && hi == 0;
        fm_search(h.L, h.code, h.C, a.data(), 0, lo, hi);
        expect(ok && lo == 0 && hi == 0, "empty_text");
    }
    // the first attempt's counter-example: pattern C in text C needs the empty-suffix row and the last byte
    expect(check_text(Text{'C'}, 0, rng) && check_text(Text{'C'}, 'C', rng), "text_C_pattern_C");
    for (uint32_t sigma : {1u, 6u, 256u}) {
        const uint32_t B = fm_block_rows(fm_is_packed(sigma));
        for (uint64_t n : {uint64_t(B) - 1, uint64_t(B), uint64_t(B) + 1, 2 * uint64_t(B), 2 * uint64_t(B) + 1}) {
            const Text t = random_text(n, sigma, rng);
            // the sentinel equals a byte of the text, and one it lacks
            const bool ok = check_text(t, t[n / 2], rng) && check_text(t, sigma == 256 ? t[0] : 200, rng);
            expect(ok, "sigma_" + std::to_string(sigma) + "_length_" + std::to_string(n));
        }
    }
    // where the primary row lies: [x1] + [x0] * a + larger bytes puts suffix 0 behind the a suffixes that start with x0: row a + 1
    for (bool packed : {true, false}) {
        const uint32_t B = fm_block_rows(packed);
        const std::string name = packed ? "packed" : "plain";
        for (int where = 0; where < 3; where++) {                            // first in a block, last in a block, SA row 0
            const uint64_t a = where == 0 ? B - 1 : where == 1 ? B - 2 : 0;
            Text t{1};
            t.insert(t.end(), a, 0);
            for (int b = 2; b < (packed ? 6 : 40); b++) t.insert(t.end(), 3, static_cast<uint8_t>(b));
            HostIndex h;
            build(t, h);
            const bool placed = h.L.primary == a + 1 && (where == 0 ? h.L.primary % B == 0 : where == 1 ? h.L.primary % B == B - 1 : h.sa[0] == 0);
            expect(placed && (h.L.packed != 0) == packed && check_text(t, 0, rng) && check_text(t, 1, rng),
                   name + "_primary_" + (where == 0 ? "first_in_block" : where == 1 ? "last_in_block" : "row_0"));
        }
    }
    // one symbol: suffix 0 is the last row, at both edges of a block
    for (uint64_t n : {uint64_t(FM_PACKED_BLOCK) - 1, uint64_t(FM_PACKED_BLOCK)}) {
        HostIndex h;
        build(Text(n, 'A'), h);
        expect(h.L.primary == n && check_text(Text(n, 'A'), 'A', rng), "one_symbol_primary_row_" + std::to_string(n));
    }
    std::printf("%s\n", failures == 0 ? "done" : "failed");
    return failures == 0 ? 0 : 1;
}
