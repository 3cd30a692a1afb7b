// fm_seed_plan.cpp -- csrc/fm_seed_plan.hpp on the host (tests/test_seeds_cpu.py builds it with ASan + UBSan): the slots and bytes of a
// seeds request with the arithmetic that gives the expected values written out, the refusals, and the capacity arithmetic.
#include <cstdio>
#include <string>

#include "fm_seed_plan.hpp"

using namespace gbwt_hip;

static int failures = 0;
static void expect(bool ok, const char *name) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
    if (!ok) failures++;
}

int main() {
    const uint64_t plenty = ~uint64_t(0);
    expect(FM_SEED_STRIDE == 16 && FM_SEED_MIN_BUFFER == 256 && FM_SEED_WORDS == 4, "constants");
    // no reads: every buffer at its least size -- 2 per item, 6 per anchor, 3 refined, 2 per end, the temporary storage, the words
    const FmSeedPlan none = fm_seed_plan(0, 0, 3, false, 0, plenty);
    expect(none.status == FmStatus::Ok && none.items == 0 && none.anchor_slots == 0 && none.end_slots == 0 && none.hit_bytes == 0 && none.scratch_bytes == (2 + 6 + 3 + 2 + 1 + 1) * 256,
           "no_reads");
    // 1000 reads of 150 bytes on both strands: 2000 items, 300000 bytes; 2000 + 300000 / 16 = 20750 anchors at most, 300000 refined ends
    const FmSeedPlan p = fm_seed_plan(1000, 150000, 3, false, 5000, plenty);
    expect(p.items == 2000 && p.anchor_slots == 20750 && p.refined_slots == 300000 && p.end_slots == 320750 && p.seed_slots == 0 && p.stride == 16 && p.strands == 3, "slots_both_strands");
    expect(p.item_bytes == 2000 * 8 + 2001 * 8 && p.anchor_bytes == 4 * 20750 * 4 + 20750 * 8 + 20751 * 8 && p.refined_bytes == 3 * 300000 * 4 && p.end_bytes == 320750 * 8 + 320751 * 8 &&
               p.temp_bytes == 5000 && p.words_bytes == 256 && p.hit_bytes == 0,
           "bytes_both_strands");
    expect(p.scratch_bytes == p.item_bytes + p.anchor_bytes + p.refined_bytes + p.end_bytes + p.temp_bytes + p.words_bytes, "scratch_is_the_sum");
    expect(fm_seed_end_slots(1000, 150000, 3) == p.end_slots && fm_seed_end_slots(1000, 150000, 1) == 1000 + 9375 + 150000, "end_slots");
    // one strand: half of everything that counts items and bytes
    const FmSeedPlan one = fm_seed_plan(1000, 150000, 2, false, 5000, plenty);
    expect(one.items == 1000 && one.anchor_slots == 10375 && one.refined_slots == 150000 && one.strands == 2 && fm_seed_plan(1000, 150000, 1, false, 5000, plenty).scratch_bytes == one.scratch_bytes,
           "slots_one_strand");
    // hits: a range and a count per seed, at most one seed per read byte and strand
    const FmSeedPlan h = fm_seed_plan(1000, 150000, 3, true, 5000, plenty);
    expect(h.seed_slots == 300000 && h.hit_bytes == 3 * 300000 * 8 && h.scratch_bytes == p.scratch_bytes + h.hit_bytes, "hits");
    // reads shorter than the stride still have an anchor each
    const FmSeedPlan tiny = fm_seed_plan(7, 7, 1, false, 0, plenty);
    expect(tiny.anchor_slots == 7 && tiny.refined_slots == 7 && tiny.end_slots == 14, "short_reads");
    // free memory: exactly the scratch is served, one byte short is refused with the bytes needed
    expect(fm_seed_plan(1000, 150000, 3, true, 5000, h.scratch_bytes).status == FmStatus::Ok, "capacity_exact_fit");
    const FmSeedPlan shortfall = fm_seed_plan(1000, 150000, 3, true, 5000, h.scratch_bytes - 1);
    expect(shortfall.status == FmStatus::Capacity && shortfall.message.find(std::to_string(h.scratch_bytes)) != std::string::npos &&
               shortfall.message.find(std::to_string(h.scratch_bytes - 1)) != std::string::npos,
           "capacity_one_byte_short");
    // the refusals that no memory changes: the strands, the reads, the bytes
    const FmSeedPlan s0 = fm_seed_plan(1, 1, 0, false, 0, plenty), s4 = fm_seed_plan(1, 1, 4, false, 0, plenty);
    expect(s0.status == FmStatus::Unsupported && s0.bad_argument && s4.status == FmStatus::Unsupported && s4.bad_argument, "strands_outside_1_to_3");
    const FmSeedPlan many = fm_seed_plan(0x7FFFFFFFull, 0, 1, false, 0, plenty);
    expect(many.status == FmStatus::Unsupported && many.bad_argument && fm_seed_plan(0x7FFFFFFEull, 0, 1, false, 0, plenty).status == FmStatus::Ok, "reads_first_refused");
    const FmSeedPlan wide = fm_seed_plan(1, uint64_t(1) << 32, 1, false, 0, plenty);
    expect(wide.status == FmStatus::Unsupported && !wide.bad_argument && wide.message.find("2^32 - 1") != std::string::npos &&
               fm_seed_plan(1, (uint64_t(1) << 32) - 1, 1, false, 0, plenty).status == FmStatus::Ok,
           "bytes_first_refused");
    expect(fm_seed_plan(1, uint64_t(1) << 32, 1, false, 0, 0).status == FmStatus::Unsupported, "width_refused_before_memory");
    std::printf("%s\n", failures == 0 ? "done" : "failed");
    return failures == 0 ? 0 : 1;
}
