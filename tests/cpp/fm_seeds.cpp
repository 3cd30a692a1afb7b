// fm_seeds.cpp -- csrc/fm_seeds.hpp on the host (tests/test_seeds_cpu.py builds it with ASan + UBSan): blocks of both layouts filled here
// through fm_layout.hpp, as tests/cpp/fm_layout.cpp fills them; fm_longest_suffix at every end of reads on both strands against a naive
// substring search over the text; the anchors; and the seed rule -- over every end, and over the anchors and the ends refined between
// them as the kernels of fm_seeds.hip walk them -- against the containment definition.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "fm_seeds.hpp"

using namespace gbwt_hip;

static int failures = 0;
static void expect(bool ok, const std::string &name) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name.c_str());
    if (!ok) failures++;
}

using Text = std::vector<uint8_t>;

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

static bool occurs(const Text &t, const uint8_t *p, size_t len) { return std::search(t.begin(), t.end(), p, p + len) != t.end(); }

// the SA range of a pattern that occurs, by looking at every suffix
static void naive_range(const Text &t, const std::vector<uint64_t> &sa, const uint8_t *p, size_t len, uint64_t &lo, uint64_t &hi) {
    lo = hi = 0;
    bool found = false;
    for (uint64_t j = 0; j < sa.size(); j++) {
        const bool starts = t.size() - sa[j] >= len && std::memcmp(t.data() + sa[j], p, len) == 0;
        if (starts && !found) { lo = j; found = true; }
        if (starts) hi = j + 1;
    }
}

static Text strand_read(const Text &read, uint32_t strand) {
    Text out(read.size());
    for (uint32_t j = 0; j < read.size(); j++) out[j] = fm_strand_byte(read.data(), static_cast<uint32_t>(read.size()), strand, j);
    return out;
}

// start[e], e in 0 .. L, of the strand's read by the definition
static std::vector<uint32_t> naive_starts(const Text &t, const Text &p) {
    std::vector<uint32_t> start(p.size() + 1, 0);
    for (uint32_t e = 1; e <= p.size(); e++) {
        uint32_t s = 0;
        while (!occurs(t, p.data() + s, e - s)) s++;
        start[e] = s;
    }
    return start;
}

using Seeds = std::vector<std::pair<uint32_t, uint32_t>>;

static Seeds seeds_by_containment(const Text &t, const Text &p, uint32_t min_length) {
    std::vector<std::pair<uint32_t, uint32_t>> occurring;
    for (uint32_t e = 1; e <= p.size(); e++)
        for (uint32_t s = 0; s < e; s++)
            if (occurs(t, p.data() + s, e - s)) occurring.emplace_back(s, e);
    Seeds kept;
    for (const auto &x : occurring) {
        bool contained = false;
        for (const auto &y : occurring) contained = contained || (y != x && y.first <= x.first && x.second <= y.second);
        if (!contained && x.second - x.first >= std::max(min_length, 1u)) kept.push_back(x);
    }
    std::sort(kept.begin(), kept.end(), [](const auto &a, const auto &b) { return a.second < b.second; });
    return kept;
}

// fm_longest_suffix at every end of one strand of a read against the definition and the naive range
static bool check_ends(const Text &t, const HostIndex &h, const Text &read, uint32_t strand) {
    const Text p = strand_read(read, strand);
    const uint32_t len = static_cast<uint32_t>(read.size());
    const std::vector<uint32_t> want = naive_starts(t, p);
    bool ok = true;
    for (uint32_t e = 0; e <= len; e++) {
        uint32_t s = 77;
        uint64_t lo = 7, hi = 7, want_lo = 0, want_hi = t.size();
        const uint32_t steps = fm_longest_suffix(h.L, h.code, h.C, read.data(), e, strand, len, s, lo, hi);
        if (want[e] != e) naive_range(t, h.sa, p.data() + want[e], e - want[e], want_lo, want_hi);
        ok = ok && s == want[e] && lo == want_lo && hi == want_hi && steps >= e - s && steps <= e - s + 1;
    }
    return ok;
}

// The seeds of one strand as the kernels find them: anchors every K ends, the ends between two anchors only where the start moved, and
// the rule over the ends whose start is known; `searched`: the ends that were
static Seeds seeds_by_anchors(const HostIndex &h, const Text &read, uint32_t strand, uint32_t K, uint32_t min_length, uint32_t &searched) {
    const uint32_t len = static_cast<uint32_t>(read.size()), anchors = fm_anchor_count(len, K);
    const uint32_t UNKNOWN = 0xFFFFFFFFu;
    std::vector<uint32_t> start(len + 2, UNKNOWN);
    const auto search = [&](uint32_t e) {
        uint64_t lo = 0, hi = 0;
        fm_longest_suffix(h.L, h.code, h.C, read.data(), e, strand, len, start[e], lo, hi);
        searched++;
    };
    for (uint32_t a = 0; a < anchors; a++) search(fm_anchor_end(len, a, K));
    for (uint32_t a = 0; a < anchors; a++) {
        const uint32_t end = fm_anchor_end(len, a, K), before = fm_anchor_before(len, a, K);
        const uint32_t refined = fm_refined_ends(before, a == 0 ? 0 : start[before], end, start[end]);
        for (uint32_t k = 0; k < refined; k++) search(before + 1 + k);
    }
    Seeds out;
    for (uint32_t e = 1; e <= len; e++) {
        if (start[e] == UNKNOWN) continue;
        // an end behind this one that was not searched has this one's start
        const uint32_t next = e == len ? 0 : (start[e + 1] == UNKNOWN ? start[e] : start[e + 1]);
        if (fm_is_seed(start[e], e, len, next, min_length)) out.emplace_back(start[e], e);
    }
    return out;
}

static Text random_text(uint64_t n, const std::string &letters, std::mt19937 &rng) {
    Text t(n);
    for (uint64_t i = 0; i < n; i++) t[i] = static_cast<uint8_t>(letters[i < letters.size() ? i : rng() % letters.size()]);
    std::shuffle(t.begin(), t.end(), rng);
    return t;
}

// a read of `len` bytes put together from pieces of the text, so that it holds several seeds
static Text pieces(const Text &t, uint32_t len, std::mt19937 &rng) {
    Text out;
    while (out.size() < len) {
        const uint32_t k = 1 + rng() % 12;
        const uint64_t at = rng() % (t.size() - k);
        out.insert(out.end(), t.begin() + at, t.begin() + at + k);
    }
    out.resize(len);
    return out;
}

int main() {
    std::mt19937 rng(20);
    const uint32_t K = FM_SEED_STRIDE;
    // the complement table and the strand's view of a read
    {
        bool ok = true;
        for (int b = 0; b < 256; b++) {
            const char *from = "ACGTacgt", *to = "TGCATGCA";
            const char *at = b ? std::strchr(from, b) : nullptr;
            ok = ok && fm_complement(static_cast<uint8_t>(b)) == static_cast<uint8_t>(at ? to[at - from] : 'N');
        }
        const Text read{'A', 'c', 'G', 'x', 'T'};
        const Text rc = strand_read(read, FM_STRAND_REVERSE);
        ok = ok && rc == Text{'A', 'N', 'C', 'G', 'T'} && strand_read(read, FM_STRAND_FORWARD) == read;
        ok = ok && fm_strand_count(1) == 1 && fm_strand_count(2) == 1 && fm_strand_count(3) == 2 && fm_strand_at(3, 0) == 1 && fm_strand_at(3, 1) == 2 && fm_strand_at(2, 0) == 2;
        expect(ok, "complement_and_strands");
    }
    // anchors: L, L - K, .. > 0, ascending by rank
    {
        bool ok = true;
        for (uint32_t stride : {1u, 4u, 16u})
            for (uint32_t len = 0; len <= 70; len++) {
                const uint32_t count = fm_anchor_count(len, stride);
                ok = ok && count == (len + stride - 1) / stride;
                for (uint32_t a = 0; a < count; a++) {
                    const uint32_t e = fm_anchor_end(len, a, stride);
                    ok = ok && e == len - (count - 1 - a) * stride && e >= 1 && e <= len && fm_anchor_before(len, a, stride) == (a == 0 ? 0 : e - stride);
                }
            }
        ok = ok && fm_refined_ends(16, 3, 32, 3) == 0 && fm_refined_ends(16, 3, 32, 4) == 15 && fm_refined_ends(0, 0, 5, 0) == 0 && fm_refined_ends(0, 0, 5, 2) == 4;
        expect(ok, "anchors");
    }
    for (bool packed : {true, false}) {
        const std::string name = packed ? "packed" : "plain";
        const Text t = random_text(packed ? 300 : 700, packed ? std::string("\0ACGT", 5) : std::string("ACGTNRYKMSWB"), rng);
        HostIndex h;
        build(t, h);
        expect((h.L.packed != 0) == packed, name + "_layout");
        // every end of reads of the lengths around the stride, both strands
        bool ends = true, rule = true, plan = true;
        for (uint32_t len : {0u, 1u, K - 1, K, K + 1, 2 * K + 1})
            for (int k = 0; k < 6; k++) {
                const Text read = pieces(t, len, rng);
                for (uint32_t strand : {FM_STRAND_FORWARD, FM_STRAND_REVERSE}) {
                    ends = ends && check_ends(t, h, read, strand);
                    const Text p = strand_read(read, strand);
                    for (uint32_t min_length : {1u, 5u}) {
                        const Seeds want = seeds_by_containment(t, p, min_length);
                        uint32_t all = 0;
                        rule = rule && seeds_by_anchors(h, read, strand, 1, min_length, all) == want && all == len;
                        for (uint32_t stride : {4u, K}) {
                            uint32_t some = 0;
                            plan = plan && seeds_by_anchors(h, read, strand, stride, min_length, some) == want && some <= len;
                        }
                    }
                }
            }
        expect(ends, name + "_longest_suffix_at_every_end");
        expect(rule, name + "_rule_is_containment");
        expect(plan, name + "_anchored_plan_is_exact");
        // a read that occurs as a whole: the anchors alone, nothing refined
        {
            const Text read(t.begin() + 20, t.begin() + 20 + 5 * K + 3);
            uint32_t searched = 0;
            const Seeds got = seeds_by_anchors(h, read, FM_STRAND_FORWARD, K, 1, searched);
            expect(got == Seeds{{0, 5 * K + 3}} && searched == 6, name + "_matching_read_searches_anchors_only");
        }
        // a byte the text lacks in the middle of a read: no match crosses it, and it costs no step
        {
            Text read = pieces(t, 2 * K + 1, rng);
            read[K] = 'z';
            bool ok = check_ends(t, h, read, FM_STRAND_FORWARD) && check_ends(t, h, read, FM_STRAND_REVERSE);
            uint32_t s = 0;
            uint64_t lo = 0, hi = 0;
            ok = ok && fm_longest_suffix(h.L, h.code, h.C, read.data(), K + 1, FM_STRAND_FORWARD, 2 * K + 1, s, lo, hi) == 0 && s == K + 1;
            ok = ok && fm_longest_suffix(h.L, h.code, h.C, read.data(), K + 2, FM_STRAND_FORWARD, 2 * K + 1, s, lo, hi) == 1 && s == K + 1 && hi > lo;
            expect(ok, name + "_absent_byte_mid_read");
        }
    }
    // the primary row inside the range: the text starts with the read, so suffix 0 is among its occurrences
    {
        Text t;
        for (int k = 0; k < 40; k++) t.insert(t.end(), {'A', 'C', 'G'});
        HostIndex h;
        build(t, h);
        const Text read{'T', 'A', 'C', 'G', 'A'};
        uint32_t s = 0;
        uint64_t lo = 0, hi = 0, want_lo = 0, want_hi = 0;
        fm_longest_suffix(h.L, h.code, h.C, read.data(), 5, FM_STRAND_FORWARD, 5, s, lo, hi);
        naive_range(t, h.sa, read.data() + 1, 4, want_lo, want_hi);
        expect(s == 1 && lo == want_lo && hi == want_hi && h.L.primary - 1 >= lo && h.L.primary - 1 < hi && check_ends(t, h, read, FM_STRAND_FORWARD) &&
                   check_ends(t, h, read, FM_STRAND_REVERSE),
               "primary_row_inside_the_range");
    }
    // an empty text: nothing occurs
    {
        HostIndex h;
        build(Text{}, h);
        const Text read{'A', 'C'};
        uint32_t s = 9;
        uint64_t lo = 7, hi = 7;
        const uint32_t steps = fm_longest_suffix(h.L, h.code, h.C, read.data(), 2, FM_STRAND_FORWARD, 2, s, lo, hi);
        expect(steps == 0 && s == 2 && lo == 0 && hi == 0, "empty_text");
    }
    std::printf("%s\n", failures == 0 ? "done" : "failed");
    return failures == 0 ? 0 : 1;
}
