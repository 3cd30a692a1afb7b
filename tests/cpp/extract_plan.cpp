// The decisions of an extraction request (csrc/extract_plan.hpp) as a program of its own, built with ASan + UBSan by
// tests/test_extract_plan_cpu.py.  One line per case, "ok <case>" or "FAIL <case>"; "done" at the end.  Small numbers, no index.
#include <cstdio>
#include <vector>

#include "extract_plan.hpp"

using namespace gbwt_hip;

static void check(const char *name, bool ok) { std::printf("%s %s\n", ok ? "ok" : "FAIL", name); }

// samples of the ten sequences of the index below
static const std::vector<uint32_t> COUNTS = {3, 3, 7, 7, 1, 1, 0, 0, 40, 40};

// ten sequences with samples (at most 40), 1 000 BWT positions per record; no uniform length, no uniform sample count
static PlanIndex index_with_samples() {
    PlanIndex ix;
    ix.sequences = 10; ix.size = 10000; ix.records = 10;
    ix.has_samples = true; ix.max_samples = 40; ix.sample_coarse = 1;
    ix.sample_counts = COUNTS.data(); ix.n_sample_counts = COUNTS.size();
    ix.orientation_pairs = true; ix.packed_blocks = true;
    return ix;
}

// the headline's shape: every sequence 1 000 nodes and 40 samples
static PlanIndex uniform_index() {
    PlanIndex ix = index_with_samples();
    ix.uniform_len = 1000; ix.uniform_samples = 40;
    return ix;
}

static IdSummary summary(bool valid, uint64_t fine, uint32_t common) { IdSummary s; s.ids_valid = valid; s.fine = fine; s.common = common; return s; }

static uint32_t stride_of(uint64_t fine, uint32_t coarse, uint32_t parts, int knob) {
    ExtractKnobs k; k.sample_stride = knob;
    PlanIndex ix = index_with_samples(); ix.sample_coarse = coarse;
    return plan_rows(k, ix, summary(true, fine, 0), 5, parts - 1, parts, 0).stride;
}

static WalkPlan walk_of(const ExtractKnobs &k, const PlanIndex &ix, uint64_t n = 5, uint32_t max_len = 1000) {
    const IdSummary ids = summary(true, 0, ix.uniform_samples);
    return plan_walk(k, ix, plan_rows(k, ix, ids, n, 0, 1, 0), true, n, 0, 1, max_len, 0);
}

int main() {
    {   // ---- id summary
        const PlanIndex ix = index_with_samples();
        const uint64_t same[] = {0, 1}, differ[] = {0, 2, 8}, invalid[] = {0, 1, 99}, zero_first[] = {6, 0};
        IdSummary s = summarize_ids(same, 2, ix);
        check("summary_same_counts", s.ids_valid && s.fine == 6 && s.common == 3);
        s = summarize_ids(differ, 3, ix);
        check("summary_counts_differ", s.ids_valid && s.fine == 3 + 7 + 40 && s.common == 0);
        s = summarize_ids(invalid, 3, ix);
        check("summary_invalid_id", !s.ids_valid && s.fine == 6 && s.common == 0);      // fine: over the valid ids
        s = summarize_ids(zero_first, 2, ix);
        check("summary_first_without_samples", s.ids_valid && s.fine == 3 && s.common == 0);
        s = summarize_ids(nullptr, 0, ix);
        check("summary_no_ids", s.ids_valid && s.fine == 0 && s.common == 0);
        PlanIndex bare = ix; bare.sample_counts = nullptr; bare.n_sample_counts = 0;
        s = summarize_ids(differ, 3, bare);
        check("summary_no_sample_counts", s.ids_valid && s.fine == 0 && s.common == 0);
    }
    {   // ---- stride: want = (fine / parts + 1 450 000) / 2 900 000, then min(2 * coarse, max(want, fine >= 524 288 ? 2 : 1))
        check("stride_below_half_a_million", stride_of(524287, 4, 1, -1) == 1);       // want 0, floor 1
        check("stride_from_half_a_million", stride_of(524288, 4, 1, -1) == 2);        // want 0, floor 2
        check("stride_by_size", stride_of(8700000, 4, 1, -1) == 3);                   // 10 150 000 / 2 900 000 = 3
        check("stride_capped", stride_of(100000000, 4, 1, -1) == 8);                  // want 34, cap 2 * 4
        check("stride_parts_divide_first", stride_of(34800000, 16, 1, -1) == 12 && stride_of(34800000, 16, 4, -1) == 3);   // 36 250 000 / 2 900 000 = 12; a quarter is 8 700 000: 3
        check("stride_set", stride_of(100000000, 4, 1, 5) == 5 && stride_of(100000000, 4, 1, 0) == 1);
        check("stride_coarse_one", stride_of(100000000, 1, 1, -1) == 1);
    }
    {   // ---- the headline's shape: all ids valid, one length, one sample count
        ExtractKnobs k; k.sample_stride = 3;
        const PlanIndex ix = uniform_index();
        const uint64_t ids5[] = {0, 2, 4, 6, 8};
        const IdSummary ids = summarize_ids(ids5, 5, ix);
        RowsPlan rows = plan_rows(k, ix, ids, 5, 0, 1, 100);
        check("headline_rows", rows.can_cut && !rows.parted && !rows.empty_part && rows.all_valid && rows.fused_offsets && !rows.defer && rows.total == 5 * 1000 &&
                                   rows.max_len == 1000 && rows.common == 40 && rows.stride == 3);
        WalkPlan w = plan_walk(k, ix, rows, ids.ids_valid, 5, 0, 1, rows.max_len, 100);
        check("headline_walk", w.segmented && !w.refused && w.same_segments && !w.needs_order && w.segments == 14 /* ceil(40 / 3) */ && w.walkers == 14 * 5 &&
                                   w.ring_slots == 64 && w.helper_naps == 4 && w.xcd_map == 1 && w.paths_per_wave == 64 && w.uniform_loop == 1 && w.uniform_len == 1000 &&
                                   w.capacity == 0 && w.both_ends == 1 && w.all4 == 1 && w.packed_blocks == 1 && w.row_piece == 32 && w.catch_up == 1);
        k.fused_offsets = 0;
        rows = plan_rows(k, ix, ids, 5, 0, 1, 100);
        w = plan_walk(k, ix, rows, ids.ids_valid, 5, 0, 1, rows.max_len, 100);
        check("headline_without_fused_offsets", rows.all_valid && !rows.fused_offsets && !rows.defer && rows.total == 5000 && rows.max_len == 1000 && w.uniform_len == 0 &&
                                                    w.same_segments && w.segments == 14 && w.walkers == 70);
    }
    {   // ---- ragged batches
        ExtractKnobs k; k.sample_stride = 3;
        const PlanIndex ix = index_with_samples();
        const uint64_t differ[] = {0, 2, 8};
        IdSummary ids = summarize_ids(differ, 3, ix);
        RowsPlan rows = plan_rows(k, ix, ids, 3, 0, 1, 100);
        WalkPlan w = plan_walk(k, ix, rows, ids.ids_valid, 3, 0, 1, 77, 100);
        check("ragged_needs_order", rows.common == 0 && !rows.defer && w.segmented && !w.same_segments && w.needs_order && w.segments == 14 /* ceil(max_samples 40 / 3) */ &&
                                        w.paths_per_wave == 64);
        const PlanIndex uniform = uniform_index();
        const uint64_t invalid[] = {0, 1, 99};
        ids = summarize_ids(invalid, 3, uniform);
        rows = plan_rows(k, uniform, ids, 3, 0, 1, 100);
        w = plan_walk(k, uniform, rows, ids.ids_valid, 3, 0, 1, 1000, 100);
        check("one_invalid_id", !rows.all_valid && !rows.fused_offsets && !rows.defer && !w.same_segments && w.needs_order && w.uniform_len == 0 && w.capacity == 0);
    }
    {   // ---- parts
        ExtractKnobs k; k.sample_stride = 3;
        const PlanIndex ix = uniform_index();
        const IdSummary ids = summary(true, 200, 40);
        bool sums = true, parted = true;
        for (uint32_t parts : {2u, 3u, 8u, 100u}) {           // 14 segments unparted (ceil(40 / 3)); 100 parts: more than there are segments
            uint64_t sum = 0;
            for (uint32_t part = 0; part < parts; part++) {
                const RowsPlan rows = plan_rows(k, ix, ids, 5, part, parts, 0);
                const WalkPlan w = plan_walk(k, ix, rows, true, 5, part, parts, 1, 0);
                parted = parted && rows.parted && !rows.all_valid && !rows.fused_offsets && w.same_segments && w.walkers == uint64_t(w.segments) * 5;
                sum += w.segments;
            }
            sums = sums && sum == 14;
        }
        check("parts_same_segments_sum", sums && parted);
        const PlanIndex ragged = index_with_samples();
        RowsPlan rows = plan_rows(k, ragged, summary(true, 50, 0), 3, 1, 3, 0);
        WalkPlan w = plan_walk(k, ragged, rows, true, 3, 1, 3, 77, 0);
        check("parts_ragged", rows.parted && w.needs_order && w.segments == 14 / 3 + 1);
        // rows that cannot be cut: every early part is n empty rows, the last part plans whole rows
        PlanIndex no_samples = ragged; no_samples.has_samples = false; no_samples.max_samples = 0; no_samples.sample_counts = nullptr; no_samples.n_sample_counts = 0;
        ExtractKnobs unsegmented; unsegmented.segments = 0;
        struct { const char *name; ExtractKnobs knobs; PlanIndex ix; uint64_t n; } uncut[] = {
            {"uncut_no_samples", ExtractKnobs{}, no_samples, 3}, {"uncut_segments_off", unsegmented, ragged, 3}, {"uncut_2_to_31_rows", ExtractKnobs{}, ragged, uint64_t(1) << 31}};
        for (const auto &c : uncut) {
            const IdSummary all = summary(true, 0, 0);
            const RowsPlan first = plan_rows(c.knobs, c.ix, all, c.n, 0, 3, 0), second = plan_rows(c.knobs, c.ix, all, c.n, 1, 3, 0), last = plan_rows(c.knobs, c.ix, all, c.n, 2, 3, 0);
            const WalkPlan whole = plan_walk(c.knobs, c.ix, last, true, c.n, 2, 3, 77, 0);
            check(c.name, first.empty_part && second.empty_part && !first.can_cut && !last.empty_part && !last.parted && !last.can_cut && !last.defer && last.stride == 1 &&
                              !whole.segmented && !whole.needs_order && whole.segments == 0 && whole.walkers == 2 * c.n);
        }
    }
    {   // ---- rows sized after the launch: only when every condition holds
        const PlanIndex ix = index_with_samples();
        const IdSummary ids = summary(true, 6, 3);
        ExtractKnobs k;
        RowsPlan rows = plan_rows(k, ix, ids, 2, 0, 1, 100);
        const WalkPlan w = plan_walk(k, ix, rows, true, 2, 0, 1, rows.max_len, 100);
        check("defer_on", rows.defer && rows.total == 100 && rows.max_len == 1 && w.capacity == 100 && w.same_segments && w.segments == 3 && w.walkers == 6);
        ExtractKnobs off; off.defer_total = 0;
        check("defer_knob_off", !plan_rows(off, ix, ids, 2, 0, 1, 100).defer);
        rows = plan_rows(k, uniform_index(), summary(true, 80, 40), 2, 0, 1, 100);
        check("defer_all_valid", rows.all_valid && !rows.defer && rows.total == 2000);
        ExtractKnobs uncut; uncut.segments = 0;
        check("defer_cannot_cut", !plan_rows(uncut, ix, ids, 2, 0, 1, 100).defer);
        check("defer_invalid_id", !plan_rows(k, ix, summary(false, 6, 0), 2, 0, 1, 100).defer);
        check("defer_counts_differ", !plan_rows(k, ix, summary(true, 10, 0), 2, 0, 1, 100).defer);
        rows = plan_rows(k, ix, ids, 2, 0, 1, 0);
        check("defer_no_rows_yet", !rows.defer && rows.total == 0 && rows.max_len == 0);
        rows = plan_rows(k, ix, ids, 2, 1, 4, 100);               // a part of rows may be deferred; it is never all_valid
        check("defer_parted", rows.parted && rows.defer && !rows.all_valid);
    }
    {   // ---- whole-row walkers (GBWT_HIP_SEGMENTS=0)
        ExtractKnobs k; k.segments = 0;
        PlanIndex ix = uniform_index();
        WalkPlan w = walk_of(k, ix);
        check("unsegmented_pairs", !w.segmented && !w.same_segments && !w.needs_order && w.segments == 0 && w.walkers == 10 && w.paths_per_wave == 16 /* (10 + 1023) / 1024 = 1 */ &&
                                       w.ring_slots == 128 && w.helper_naps == 1 && w.xcd_map == 0 && w.both_ends == 1);
        ix.orientation_pairs = false;
        w = walk_of(k, ix);
        check("unsegmented_one_end", w.walkers == 5 && w.both_ends == 0 && w.paths_per_wave == 16);
        check("unsegmented_paths_per_wave", walk_of(k, ix, 40000).paths_per_wave == 40 /* 41 023 / 1024 */ && walk_of(k, ix, 100000).paths_per_wave == 64 /* 98, clamped */);
        k.paths_per_wave = 8;
        ExtractKnobs segmented; segmented.paths_per_wave = 8;
        check("tuned_paths_per_wave", walk_of(k, ix).paths_per_wave == 8 && walk_of(segmented, ix).paths_per_wave == 8 && walk_of(segmented, ix).segmented);
    }
    {   // ---- a lean handle
        ExtractKnobs whole; whole.segments = 0;
        PlanIndex lean = uniform_index(); lean.lean = true;
        check("lean_refuses_whole_rows", walk_of(whole, lean, 5, 1000).refused && !walk_of(whole, uniform_index(), 5, 1000).refused);
        check("lean_serves_empty_rows", !walk_of(whole, lean, 5, 0).refused && !walk_of(ExtractKnobs{}, lean, 5, 1000).refused);
        PlanIndex lean_unpacked = lean; lean_unpacked.packed_blocks = false;
        PlanIndex unpacked = uniform_index(); unpacked.packed_blocks = false;
        ExtractKnobs two; two.catch_up = 2;
        ExtractKnobs seven; seven.catch_up = 7;
        ExtractKnobs none; none.catch_up = 0;
        ExtractKnobs no_packed; no_packed.packed_blocks = 0;
        check("catch_up_lean", walk_of(ExtractKnobs{}, lean).catch_up == 2 && walk_of(ExtractKnobs{}, lean_unpacked).catch_up == 0 && walk_of(no_packed, lean).catch_up == 0);
        check("catch_up_two", walk_of(two, uniform_index()).catch_up == 2 && walk_of(two, unpacked).catch_up == 1 && walk_of(two, lean_unpacked).catch_up == 0);
        check("catch_up_capped", walk_of(seven, uniform_index()).catch_up == 2 && walk_of(none, uniform_index()).catch_up == 0 && walk_of(none, lean).catch_up == 0);
    }
    {   // ---- clamps of ring and headroom
        const PlanIndex ix = uniform_index();
        ExtractKnobs k; k.ring_slots = 32;
        check("ring_holds_two_pieces", walk_of(k, ix).ring_slots == 64 && walk_of(k, ix).row_piece == 32);
        k.row_piece = 16;
        check("ring_32_with_piece_16", walk_of(k, ix).ring_slots == 32);
        ExtractKnobs h; h.headroom = 32;
        check("headroom_ring_minus_piece", walk_of(h, ix).ring_slots == 64 && walk_of(h, ix).headroom == 32);          // 64 - 32
        h.ring_slots = 32; h.row_piece = 16;
        check("headroom_clamped_to_piece", walk_of(h, ix).headroom == 16);                                              // 32 - 16
        h.row_piece = 0;
        check("headroom_without_pieces", walk_of(h, ix).ring_slots == 32 && walk_of(h, ix).headroom == 31);             // ring - 1
    }
    {   // ---- look-ahead of mixed waves: below 512 BWT positions per record
        PlanIndex ix = uniform_index();
        ix.size = 5110;
        check("gather_reach_511", walk_of(ExtractKnobs{}, ix).gather_reach == 1);
        ix.size = 5120;
        check("gather_reach_512", walk_of(ExtractKnobs{}, ix).gather_reach == 0);
        ix.size = 5110; ix.records = 0;
        check("gather_reach_no_records", walk_of(ExtractKnobs{}, ix).gather_reach == 0);
        ix.records = 10;
        ExtractKnobs five; five.gather_reach = 5;
        ExtractKnobs off; off.gather_reach = 0;
        check("gather_reach_knob", walk_of(five, ix).gather_reach == 5 && walk_of(off, ix).gather_reach == 0);
    }
    {   // ---- the pool-output walk
        PlanIndex ix = index_with_samples();
        check("pool_blocks", plan_pool_blocks(ix, 5, 256) == 9990 / 256 + 5 + 1);       // 39 + 6
        ix.size = 3;
        check("pool_blocks_size_below_sequences", plan_pool_blocks(ix, 5, 256) == 6);
        ExtractKnobs k;
        check("pool_paths_per_wave", plan_pool_paths_per_wave(k, 5) == 32 && plan_pool_paths_per_wave(k, 40000) == 40 && plan_pool_paths_per_wave(k, 100000) == 64);
        k.paths_per_wave = 8;
        check("pool_paths_per_wave_tuned", plan_pool_paths_per_wave(k, 5) == 8);
    }
    std::printf("done\n");
    return 0;
}
