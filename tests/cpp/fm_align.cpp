// fm_align.cpp -- csrc/fm_align.hpp on the host (tests/test_align_cpu.py builds it with ASan + UBSan and runs it as a program): the banded DP
// row by row over host arrays with the very functions the kernel calls -- the cells of a row that exist, the cell rule, the deletion chain
// as a prefix minimum of skewed values, the directions of 64 cells packed from two masks, the walk back and the CIGAR entries.  It prints
// its inputs and its results; the test runs the yardstick (tests/align_expect.py) over the printed inputs and compares.  The text of a
// case is the window T[base, base + |text|) of a text that may start far up: a member with y above 2^32 - 200 costs no memory.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "fm_align.hpp"

using namespace gbwt_hip;

struct Member { uint64_t y; uint32_t x, w; };

static uint64_t state = 2024;
static uint32_t next(uint32_t below) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>((state >> 33) % below);
}

static std::vector<uint8_t> bases(size_t n) {
    std::vector<uint8_t> out(n);
    for (uint8_t &b : out) b = "ACGT"[next(4)];
    return out;
}

static void print(const std::string &name, const char *what, const std::vector<uint8_t> &v) {
    std::printf("%s.%s", name.c_str(), what);
    for (uint8_t a : v) std::printf(" %u", a);
    std::printf("\n");
}

// lo, hi and the members are text positions; text[t] = T[base + t]
static void run(const std::string &name, const std::vector<uint8_t> &read, const std::vector<uint8_t> &text, uint64_t base, const std::vector<Member> &members, uint32_t band,
                uint32_t max_width, uint64_t lo, uint64_t hi) {
    std::printf("%s.options %u %u %llu %llu %llu\n", name.c_str(), band, max_width, static_cast<unsigned long long>(lo), static_cast<unsigned long long>(hi),
                static_cast<unsigned long long>(base));
    print(name, "read", read);
    print(name, "text", text);
    std::printf("%s.members", name.c_str());
    int64_t dmin = 0, dmax = 0;
    for (size_t t = 0; t < members.size(); t++) {
        std::printf(" %llu,%u,%u", static_cast<unsigned long long>(members[t].y), members[t].x, members[t].w);
        const int64_t d = fm_align_diagonal(members[t].y, members[t].x);
        if (t == 0 || d < dmin) dmin = d;
        if (t == 0 || d > dmax) dmax = d;
    }
    std::printf("\n");
    const int64_t d0 = fm_align_d0(dmin, band);
    const uint64_t width = fm_align_width(dmin, dmax, band);
    if (width > fm_align_max_width(max_width)) {
        std::printf("%s.result %u %llu %u 0 0\n%s.cigar\n", name.c_str(), GBWT_HIP_ALIGN_WIDE, static_cast<unsigned long long>(width), FM_ALIGN_INF, name.c_str());
        return;
    }
    const uint32_t W = static_cast<uint32_t>(width), L = static_cast<uint32_t>(read.size()), words = fm_align_row_words(W), chunks = (W + 63) / 64;
    const auto text_at = [&](uint64_t j) { return text.at(j - base); };
    std::vector<uint32_t> h(W), directions(static_cast<size_t>(L) * words + 1, 0xDEADBEEFu);
    int32_t first = 0, last = -1;
    fm_align_row_range(d0, W, lo, hi, 0, first, last);
    for (uint32_t k = 0; k < W; k++) h[k] = static_cast<int32_t>(k) >= first && static_cast<int32_t>(k) <= last ? 0u : FM_ALIGN_INF;
    for (uint32_t i = 1; i <= L; i++) {
        fm_align_row_range(d0, W, lo, hi, i, first, last);
        std::vector<uint32_t> row(W), direction(W, FM_ALIGN_DIAGONAL);
        uint32_t running = FM_ALIGN_INF;                                          // the prefix minimum of the skewed values
        for (uint32_t k = 0; k < W; k++) {
            const bool exists = static_cast<int32_t>(k) >= first && static_cast<int32_t>(k) <= last;
            const uint32_t above = k + 1 < W ? h[k + 1] : FM_ALIGN_INF;
            const uint64_t j = static_cast<uint64_t>(d0 + static_cast<int64_t>(i) + static_cast<int64_t>(k));
            const uint8_t t = exists && h[k] != FM_ALIGN_INF ? text_at(j - 1) : 0;
            const uint32_t a = exists ? fm_align_cell(h[k], read[i - 1] != t, above, direction[k]) : FM_ALIGN_INF;
            const uint32_t skewed = fm_align_skew(a, k);
            if (skewed < running) running = skewed;
            const uint32_t value = exists ? fm_align_unskew(running, k) : FM_ALIGN_INF;
            // the prefix minimum is the chain of fm_align_delete: both must give the cell
            uint32_t chained_direction = direction[k];
            const uint32_t chained = exists ? fm_align_delete(a, k >= 1 ? row[k - 1] : FM_ALIGN_INF, chained_direction) : FM_ALIGN_INF;
            if (value < a) direction[k] = FM_ALIGN_DELETION;
            if (chained != value || (value != FM_ALIGN_INF && chained_direction != direction[k])) std::printf("FAIL %s: the chain and the prefix minimum differ at (%u, %u)\n", name.c_str(), i, k);
            row[k] = value;
        }
        for (uint32_t c = 0; c < chunks; c++) {                                   // two masks of 64 cells, four words
            uint64_t low_bits = 0, high_bits = 0;
            for (uint32_t lane = 0; lane < 64 && c * 64 + lane < W; lane++) {
                low_bits |= static_cast<uint64_t>(direction[c * 64 + lane] & 1u) << lane;
                high_bits |= static_cast<uint64_t>((direction[c * 64 + lane] >> 1) & 1u) << lane;
            }
            for (uint32_t word = 0; word < 4 && 4 * c + word < words; word++) directions[static_cast<size_t>(i - 1) * words + 4 * c + word] = fm_align_direction_word(low_bits, high_bits, word);
        }
        for (uint32_t k = 0; k < W; k++)
            if (fm_align_direction_at(directions[static_cast<size_t>(i - 1) * words + k / 16], k) != direction[k]) std::printf("FAIL %s: direction (%u, %u) does not unpack\n", name.c_str(), i, k);
        h = row;
    }
    if (directions.back() != 0xDEADBEEFu) std::printf("FAIL %s: a word behind the directions was written\n", name.c_str());
    uint64_t key = ~uint64_t(0);
    for (uint32_t k = 0; k < W; k++) key = fm_align_end_key(h[k], k) < key ? fm_align_end_key(h[k], k) : key;
    const uint32_t distance = static_cast<uint32_t>(key >> 32), k_end = static_cast<uint32_t>(key);
    if (distance == FM_ALIGN_INF) {
        std::printf("%s.result %u %u %u 0 0\n%s.cigar\n", name.c_str(), GBWT_HIP_ALIGN_NONE, W, FM_ALIGN_INF, name.c_str());
        return;
    }
    const uint32_t bound = static_cast<uint32_t>(fm_align_cigar_bound(L));
    std::vector<uint32_t> entries(bound);
    uint32_t k_start = 0;
    const uint32_t count = fm_align_trace(L, W, d0, k_end, directions.data(), [&](uint32_t i) { return read[i]; }, text_at, entries.data(), bound, k_start);
    std::printf("%s.result %u %u %u %llu %llu\n", name.c_str(), GBWT_HIP_ALIGN_OK, W, distance, static_cast<unsigned long long>(d0 + static_cast<int64_t>(k_start)),
                static_cast<unsigned long long>(d0 + static_cast<int64_t>(L) + static_cast<int64_t>(k_end)));
    std::printf("%s.cigar", name.c_str());
    for (uint32_t e = 0; e < count; e++) std::printf(" %u", entries[bound - count + e]);
    std::printf("\n");
}

// `read` = text[from, from + n) with a base replaced, some deleted and some inserted
static std::vector<uint8_t> edited(const std::vector<uint8_t> &text, size_t from, size_t n, size_t deleted, size_t inserted) {
    std::vector<uint8_t> read(text.begin() + from, text.begin() + from + n);
    read[n / 4] = read[n / 4] == 'A' ? 'C' : 'A';
    read.erase(read.begin() + n / 2, read.begin() + n / 2 + deleted);
    for (size_t k = 0; k < inserted; k++) read.insert(read.begin() + 3 * n / 4, "ACGT"[next(4)]);
    return read;
}

int main() {
    static_assert(sizeof(gbwt_hip_fm_alignment) == 40 && sizeof(gbwt_hip_fm_align_options) == 24, "the structs of include/gbwt_hip.h");
    const std::vector<uint8_t> text = bases(700);
    const uint64_t n = text.size();
    // edits inside the band: a replaced base, 3 deleted, 2 inserted; two members on diagonals 3 apart
    run("edits", edited(text, 100, 120, 3, 2), text, 0, {{100, 0, 30}, {163, 60, 20}}, 8, 0, 0, n);
    // the same far up in a text: y above 2^32 - 200, d is signed 64-bit and y + w passes 2^32
    const uint64_t base = 0x100000000ull - 200;
    run("high", edited(text, 100, 120, 3, 2), text, base, {{base + 100, 0, 30}, {base + 163, 60, 20}}, 8, 0, base, base + n);
    // a band that reaches below text position 0: d0 = 2 - 5 - 8 < 0, and the first read bytes are insertions or the start moves
    run("below", edited(text, 0, 90, 0, 0), text, 0, {{2, 5, 20}}, 8, 0, 0, n);
    std::vector<uint8_t> overhang(text.begin(), text.begin() + 60);
    overhang.insert(overhang.begin(), {'T', 'T', 'G'});
    run("below_start", overhang, text, 0, {{0, 3, 60}}, 4, 0, 0, n);
    // segments inside the text: bounds cut the band on both sides
    run("bounded", edited(text, 300, 100, 2, 0), text, 0, {{300, 0, 40}}, 16, 0, 295, 396);
    run("none", edited(text, 300, 100, 0, 0), text, 0, {{300, 0, 40}}, 8, 0, 295, 380);
    // widths at the edges of a lane chunk and at the most: 1, 63, 64, 65, 128, 129 and FM_ALIGN_MAX_WIDTH
    run("width_1", std::vector<uint8_t>(text.begin() + 200, text.begin() + 260), text, 0, {{200, 0, 60}}, 0, 1, 0, n);
    run("width_63", edited(text, 200, 100, 4, 0), text, 0, {{200, 0, 30}}, 31, 63, 0, n);
    run("width_64", edited(text, 200, 100, 4, 0), text, 0, {{200, 0, 30}, {265, 64, 20}}, 31, 64, 0, n);
    run("width_65", edited(text, 200, 100, 0, 5), text, 0, {{200, 0, 30}}, 32, 65, 0, n);
    run("width_128", edited(text, 200, 100, 4, 3), text, 0, {{200, 0, 30}, {265, 64, 20}}, 63, 128, 0, n);
    run("width_129", edited(text, 200, 100, 4, 3), text, 0, {{200, 0, 30}}, 64, 129, 0, n);
    run("width_most", edited(text, 200, 80, 2, 2), text, 0, {{200, 0, 30}, {261, 60, 20}}, 511, FM_ALIGN_MAX_WIDTH, 0, n);
    run("wide", edited(text, 200, 80, 2, 2), text, 0, {{200, 0, 30}, {261, 60, 20}}, 511, FM_ALIGN_MAX_WIDTH - 1, 0, n);
    run("wide_default", edited(text, 200, 80, 2, 2), text, 0, {{200, 0, 30}}, 128, 0, 0, n);
    // packing
    std::printf("entry %u %u %u\n", fm_cigar_entry(150, FM_CIGAR_EQ), fm_cigar_entry(1, FM_CIGAR_X), fm_cigar_entry(FM_ALIGN_MAX_READ, FM_CIGAR_I));
    std::printf("tile %llu %d %d\n", static_cast<unsigned long long>(FM_ALIGN_TILE_BYTES), fm_align_in_tile(FM_ALIGN_TILE_BYTES / 8, 17) ? 1 : 0,
                fm_align_in_tile(FM_ALIGN_TILE_BYTES / 8 + 1, 17) ? 1 : 0);
    std::printf("done\n");
    return 0;
}
