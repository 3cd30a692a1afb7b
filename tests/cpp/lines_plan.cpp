// The decisions of a GFA lines request (csrc/lines_plan.hpp) as a program of its own, built with ASan + UBSan by
// tests/test_lines_plan_cpu.py.  One line per case, "ok <case>" or "FAIL <case>"; "done" at the end.  Numbers only, no index.
#include <cstdio>
#include <string>
#include <vector>

#include "lines_plan.hpp"

using namespace gbwt_hip;

static void check(const std::string &name, bool ok) { std::printf("%s %s\n", ok ? "ok" : "FAIL", name.c_str()); }

// regions of a buffer as [begin, end) in bytes, in the order they are given: ascending and pairwise disjoint, the last one ends at `bytes`
struct Region { uint64_t word, count, width; };     // offset in 64-bit words, elements, bytes per element
static bool regions_fit(const std::vector<Region> &regions, uint64_t bytes) {
    uint64_t end = 0;
    for (const Region &r : regions) {
        const uint64_t begin = r.word * 8;
        if (begin < end || begin % r.width != 0) return false;         // overlaps the one before it, or is not aligned for its elements
        end = begin + r.count * r.width;
    }
    return end == bytes;
}

static bool lines_layout_ok(uint64_t n, uint64_t cap) {
    const LinesLayout l = lines_layout(n, cap);
    // the sizes a request reserved before the layout existed
    const uint64_t a = 2 * n * 8, first = 2 * (n + 1) * 8, chunks = (3 * cap + 3 * (cap + 1)) * 8 + (cap + 1) * 4;
    return l.a_bytes == a && l.chunk_first_bytes == first && l.chunks_bytes == chunks &&
           regions_fit({{l.line_len, n, 8}, {l.line_end, n, 8}}, a) &&
           regions_fit({{l.chunk_first, n + 1, 8}, {l.chunk_counts, n, 8}}, first - 8) &&      // (counts has n entries: the last word is spare)
           regions_fit({{l.chunk_text, cap, 8}, {l.chunk_seq, cap, 8}, {l.chunk_bad, cap, 8}, {l.text_before, cap + 1, 8}, {l.seq_before, cap + 1, 8},
                        {l.bad_before, cap + 1, 8}, {l.chunk_path, cap + 1, 4}}, chunks) &&
           (l.chunk_path * 8) % 4 == 0;
}

static bool tokens_layout_ok(uint64_t n, uint64_t cap) {
    const TokensLayout l = tokens_layout(n, cap);
    const uint64_t a = 2 * (n + 1) * 8, first = 2 * (n + 1) * 8, chunks = (2 * cap + 2 * (cap + 1)) * 8 + (cap + 1) * 4;
    return l.a_bytes == a && l.chunk_first_bytes == first && l.chunks_bytes == chunks &&
           regions_fit({{l.row_tokens, n + 1, 8}, {l.row_start, n + 1, 8}}, a) &&
           regions_fit({{l.chunk_first, n + 1, 8}, {l.chunk_counts, n, 8}}, first - 8) &&
           regions_fit({{l.chunk_tokens, cap, 8}, {l.chunk_bad, cap, 8}, {l.tokens_before, cap + 1, 8}, {l.bad_before, cap + 1, 8}, {l.chunk_path, cap + 1, 4}}, chunks) &&
           (l.chunk_path * 8) % 4 == 0;
}

static std::vector<uint64_t> batches(const std::vector<uint64_t> &ids, const std::vector<uint32_t> &seq_len, uint64_t token, uint64_t budget, uint64_t fallback = 4096) {
    std::vector<uint64_t> cuts;
    for (uint64_t b0 = 0; b0 < ids.size();) {
        const uint64_t nb = next_batch(ids.data(), ids.size(), b0, seq_len.data(), seq_len.size(), token, budget, fallback);
        if (nb == 0) return {};                                        // (would never end)
        cuts.push_back(nb);
        b0 += nb;
    }
    return cuts;
}

int main() {
    {   // ---- scratch layouts: (rows, chunk bound)
        const uint64_t shapes[4][2] = {{1, 1}, {1, 2}, {3, 7}, {uint64_t(1) << 20, (uint64_t(1) << 31) - 1}};
        for (const auto &s : shapes) {
            const std::string at = std::to_string(s[0]) + "_" + std::to_string(s[1]);
            check("lines_layout_" + at, lines_layout_ok(s[0], s[1]));
            check("tokens_layout_" + at, tokens_layout_ok(s[0], s[1]));
        }
        const LinesLayout l = lines_layout(3, 7);      // words: 7 + 7 + 7 + 8 + 8 + 8 = 45 in front of the 32-bit array; 45 * 8 + 8 * 4 = 392 bytes
        check("lines_layout_words", l.chunk_seq == 7 && l.chunk_bad == 14 && l.text_before == 21 && l.seq_before == 29 && l.bad_before == 37 && l.chunk_path == 45 &&
                                        l.chunks_bytes == 392 && l.line_end == 3 && l.chunk_counts == 4);
        const TokensLayout t = tokens_layout(3, 7);    // 7 + 7 + 8 + 8 = 30 words; 30 * 8 + 8 * 4 = 272 bytes
        check("tokens_layout_words", t.chunk_bad == 7 && t.tokens_before == 14 && t.bad_before == 22 && t.chunk_path == 30 && t.chunks_bytes == 272 && t.row_start == 4);
        int probe[4] = {0, 0, 0, 0};
        check("scratch_at", scratch_at<int>(probe, 1) == probe + 2 && scratch_at<uint64_t>(probe, 0) == reinterpret_cast<uint64_t *>(probe));   // offsets count 64-bit words
    }
    {   // ---- chunk bound: total / LINE_CHUNK + n
        check("chunks_cap_total_0", chunks_cap(0, 5).chunks == 5 && !chunks_cap(0, 5).refused);
        check("chunks_cap_below_a_chunk", chunks_cap(LINE_CHUNK - 1, 5).chunks == 5);
        check("chunks_cap_a_chunk", chunks_cap(LINE_CHUNK, 5).chunks == 6);
        check("chunks_cap_above_a_chunk", chunks_cap(LINE_CHUNK + 1, 5).chunks == 6);
        // 2^31 - 1 chunks are served, 2^31 are not: with 7 rows that is total / 4096 = 2^31 - 8, reached at (2^31 - 8) * 4096 and left at (2^31 - 7) * 4096
        const uint64_t last = ((uint64_t(1) << 31) - 8) * LINE_CHUNK + (LINE_CHUNK - 1);
        check("chunks_cap_last_served", chunks_cap(last, 7).chunks == 0x7FFFFFFFull && !chunks_cap(last, 7).refused);
        check("chunks_cap_first_refused", chunks_cap(last + 1, 7).chunks == 0x80000000ull && chunks_cap(last + 1, 7).refused);
        check("chunks_cap_rows_alone", !chunks_cap(0, 0x7FFFFFFFull).refused && chunks_cap(0, 0x80000000ull).refused);
        check("refusal_texts", std::string(LINES_TOO_MANY_CHUNKS) == "too many line chunks in one batch: format fewer paths per call" &&
                                   std::string(TOKENS_TOO_MANY_CHUNKS) == "too many chunks in one batch: ask for fewer paths per call");
    }
    {   // ---- sizing variant: (translated, lc_state)
        check("sizing_cached", line_sizing(false, 1) == LineSizing::Cached);
        check("sizing_plain", line_sizing(false, -1) == LineSizing::Plain && line_sizing(false, 0) == LineSizing::Plain);
        check("sizing_translated", line_sizing(true, -1) == LineSizing::Translated);
        check("sizing_translated_ignores_cache", line_sizing(true, 1) == LineSizing::Translated);
    }
    {   // ---- passes of a whole file: (path mode, generic sample present)
        using P = std::vector<LinePass>;
        check("passes_default_with_ref", gfa_passes(0, true) == P{{0, 0}, {1, 1}});      // P-lines of the generic sample, W-lines of the others
        check("passes_default_without_ref", gfa_passes(0, false) == P{{1, 1}});          // every path is one of the others
        check("passes_pan_sn_with_ref", gfa_passes(1, true) == P{{2, 2}});
        check("passes_pan_sn_without_ref", gfa_passes(1, false) == P{{2, 2}});
        check("passes_ref_only_with_ref", gfa_passes(2, true) == P{{0, 0}});
        check("passes_ref_only_without_ref", gfa_passes(2, false).empty());
    }
    {   // ---- widest token: digits of the largest node id (or the longest segment name) + 2
        check("token_digits", token_width_bound(0, false, 0) == 3 && token_width_bound(9, false, 0) == 3 && token_width_bound(10, false, 0) == 4 &&
                                  token_width_bound(99999, false, 0) == 7 && token_width_bound(~uint64_t(0), false, 0) == 22);
        check("token_names", token_width_bound(99999, true, 0) == 2 && token_width_bound(99999, true, 11) == 13);
    }
    {   // ---- batches: the estimate of path p is 128 + token * seq_len[2 p]; token 6 here, so a path of 10 nodes is 188 bytes
        const std::vector<uint64_t> ids = {0, 1, 2, 3, 4};
        const std::vector<uint32_t> tens = {10, 0, 10, 0, 10, 0, 10, 0, 10, 0};
        using B = std::vector<uint64_t>;
        check("batch_larger_than_budget_goes_alone", batches({0, 1, 2}, {1000, 0, 10, 0, 10, 0}, 6, 400) == B{1, 2});          // 6 128 bytes alone; then 188 + 188 <= 400
        check("batch_exact_fit", batches(ids, tens, 6, 2 * 188) == B{2, 2, 1});
        check("batch_one_byte_over", batches(ids, tens, 6, 2 * 188 - 1) == B{1, 1, 1, 1, 1});
        check("batch_last_short", batches(ids, tens, 6, 3 * 188) == B{3, 2});
        std::vector<uint64_t> many(10000);
        for (size_t i = 0; i < many.size(); i++) many[i] = i;
        check("batch_without_lengths_by_count", batches(many, {}, 6, 1) == B{4096, 4096, 10000 - 2 * 4096});
        check("batch_beyond_the_lengths_estimates_0", batches({0, 7, 8, 1}, {10, 0, 10, 0}, 6, 2 * 188) == B{4});              // 188 + 0 + 0 + 188
        check("batch_first_always_goes_in", next_batch(ids.data(), ids.size(), 4, tens.data(), tens.size(), 6, 1, 4096) == 1 &&
                                                 next_batch(ids.data(), ids.size(), 5, tens.data(), tens.size(), 6, 1, 4096) == 0);      // (nothing left: nothing)
    }
    std::printf("done\n");
    return 0;
}
