// fm_chains.cpp -- csrc/fm_chains.hpp on the host (tests/test_chains_cpu.py builds it with ASan + UBSan and runs it as a program): the DP and
// the peeling over host arrays with the very functions the kernels call.  It prints its inputs and its results; the test runs the yardstick
// (tests/chain_expect.py) over the printed inputs and compares.  The cases hold equal-score ties (the packed key must pick the largest j),
// scores that go negative (c is signed), windows cut by max_gap and by segments, and a min_score that drops chains.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "fm_chains.hpp"

using namespace gbwt_hip;

struct Item {
    std::vector<uint32_t> y, x, w, seg, seg_start;
};

static void print(const std::string &name, const char *what, const std::vector<uint32_t> &v) {
    std::printf("%s.%s", name.c_str(), what);
    for (uint32_t a : v) std::printf(" %lld", a == FM_CHAIN_NONE ? -1ll : static_cast<long long>(a));
    std::printf("\n");
}

// segments of `width` text positions each
static Item item_of(std::vector<std::pair<uint32_t, uint32_t>> yx, const std::vector<uint32_t> &lengths, uint32_t width) {
    std::sort(yx.begin(), yx.end());
    yx.erase(std::unique(yx.begin(), yx.end()), yx.end());
    Item it;
    for (size_t k = 0; k < yx.size(); k++) {
        it.y.push_back(yx[k].first);
        it.x.push_back(yx[k].second);
        it.w.push_back(lengths[k % lengths.size()]);
        it.seg.push_back(width ? yx[k].first / width : 0);
        it.seg_start.push_back(width ? yx[k].first / width * width : 0);
    }
    return it;
}

static void run(const std::string &name, const Item &it, uint32_t max_gap, uint32_t max_skew, uint32_t gap_cost, uint32_t min_score) {
    const FmChainParams P = fm_chain_params(max_gap, max_skew, gap_cost, min_score);
    const uint32_t n = static_cast<uint32_t>(it.y.size());
    std::printf("%s.options %u %u %u %u\n", name.c_str(), max_gap, max_skew, gap_cost, min_score);
    print(name, "y", it.y); print(name, "x", it.x); print(name, "w", it.w); print(name, "seg", it.seg);
    // the DP: every j in front of i; the window of the kernel is what fm_chain_admissible lets through
    std::vector<uint32_t> f(n), pred(n);
    uint64_t pairs = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t low = fm_chain_low(it.y[i], it.seg_start[i], P.max_gap);
        uint64_t best = 0;
        for (uint32_t j = 0; j < i; j++) best = fm_chain_step(best, j, it.y[j], it.x[j], f[j], it.y[i], it.x[i], it.w[i], low, P, pairs);
        fm_chain_result(best, it.w[i], f[i], pred[i]);
    }
    print(name, "f", f); print(name, "pred", pred);
    std::printf("%s.pairs %llu\n", name.c_str(), static_cast<unsigned long long>(pairs));
    // the peeling: the visiting order by the sort key, stable
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return fm_chain_visit_key(0, f[a]) < fm_chain_visit_key(0, f[b]); });
    std::vector<uint8_t> used(n, 0);
    std::vector<uint32_t> member_slot(n, 0), member_pos(n, 0);
    std::printf("%s.chains", name.c_str());
    for (uint32_t t = 0; t < n; t++) {
        const uint32_t head = order[t];
        if (used[head]) continue;
        int64_t score = 0;
        uint32_t tail = head;
        const uint32_t members = fm_chain_peel(head, t, f.data(), pred.data(), used.data(), member_slot.data(), member_pos.data(), score, tail);
        if (!fm_chain_reported(score, P)) continue;
        const gbwt_hip_fm_chain c = fm_chain_summary(it.y[tail], it.x[tail], it.y[head], it.x[head], it.w[head], static_cast<uint32_t>(score), members, 1, it.seg[head]);
        std::printf(" %llu,%llu,%u,%u,%u,%u,%u,%u", static_cast<unsigned long long>(c.text_start), static_cast<unsigned long long>(c.text_end), c.read_start, c.read_end, c.score,
                    c.matches, c.strand, c.path);
        // the members by ascending index: those whose slot is t, placed from the end of the row by their distance from the head
        std::vector<uint32_t> row(members);
        for (uint32_t k = 0; k < n; k++)
            if (used[k] && member_slot[k] == t) row[members - 1 - member_pos[k]] = k;
        std::printf(":");
        for (uint32_t k = 0; k < members; k++) std::printf("%s%u", k ? "+" : "", row[k]);
    }
    std::printf("\n");
}

int main() {
    static_assert(sizeof(gbwt_hip_fm_chain) == 40 && sizeof(gbwt_hip_fm_chain_match) == 16 && sizeof(gbwt_hip_fm_chain_options) == 32, "the structs of include/gbwt_hip.h");
    // a periodic item: two seeds of 6 bytes at x = 0 and x = 7 with hits at every even y: dy 6 and dy 8 both give 11
    std::vector<std::pair<uint32_t, uint32_t>> periodic;
    for (uint32_t k = 0; k < 60; k++) { periodic.push_back({2 * k, 0}); periodic.push_back({2 * k, 7}); }
    run("ties", item_of(periodic, {6}, 0), 400, 8, 1, 1);
    run("ties_free", item_of(periodic, {6}, 0), 400, 8, 0, 1);
    run("ties_cut", item_of(periodic, {6}, 0), 20, 2, 3, 12);
    // a costly skew: c goes far below zero and must not wrap
    run("signed", item_of(periodic, {6, 9, 4}, 0), 0, 0, 4000000, 1);
    // scattered matches, with and without segments
    uint64_t state = 12345;
    const auto next = [&state](uint32_t below) { state = state * 6364136223846793005ull + 1442695040888963407ull; return static_cast<uint32_t>((state >> 33) % below); };
    std::vector<std::pair<uint32_t, uint32_t>> scattered;
    for (int k = 0; k < 150; k++) {
        const uint32_t diagonal = 100 * next(6), x = next(120);
        scattered.push_back({diagonal + x + next(4), x});
    }
    run("scattered", item_of(scattered, {5, 12, 7, 20, 9}, 0), 60, 5, 1, 1);
    run("segments", item_of(scattered, {5, 12, 7, 20, 9}, 128), 60, 5, 1, 10);
    run("defaults", item_of(scattered, {5, 12, 7, 20, 9}, 0), 0, 0, 2, 0);
    // y at the top of the range: low saturates at 0 and nothing overflows
    std::vector<std::pair<uint32_t, uint32_t>> high;
    for (uint32_t k = 0; k < 20; k++) high.push_back({0xFFFFFFF0u - 40 * (19 - k), 30 * k});
    run("high", item_of(high, {25}, 0), 0x7FFFFFFFu, 0x7FFFFFFFu, 1, 1);
    run("empty", item_of({}, {1}, 0), 0, 0, 1, 1);
    std::printf("done\n");
    return 0;
}
