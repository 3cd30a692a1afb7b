// fm_align_plan.cpp -- csrc/fm_align_plan.hpp on the host (tests/test_align_cpu.py builds it with ASan + UBSan): the bytes of the alignment's
// scratch with the arithmetic that gives the expected values written out, the refusal, and the capacity arithmetic.
#include <cstdio>
#include <string>

#include "fm_align_plan.hpp"

using namespace gbwt_hip;

static int failures = 0;
static void expect(bool ok, const char *name) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
    if (!ok) failures++;
}

int main() {
    const uint64_t plenty = ~uint64_t(0);
    expect(FM_ALIGN_MIN_BUFFER == 256 && FM_ALIGN_WORDS == 8 && FM_ALIGN_TASK_BYTES == 80 && FM_ALIGN_TILE_BYTES == 8192 && FM_ALIGN_MAX_WIDTH == 1024 &&
               FM_ALIGN_MAX_ALIGNMENTS == 0x7FFFFFFFull,
           "constants");
    // the tile: 1024 rows of 2 words fit, one row more does not; the CIGAR bound is 2 L
    expect(fm_align_in_tile(1024, 17) && fm_align_in_tile(1024, 32) && !fm_align_in_tile(1025, 17) && !fm_align_in_tile(1024, 33) && fm_align_in_tile(2, 1024) && !fm_align_in_tile(33, 1024),
           "tile");
    expect(fm_align_cigar_bound(150) == 300 && fm_align_cigar_bound(0) == 0, "cigar_bound");
    // nothing to do: every buffer at its least size -- 3 per item, the tasks, 5 sizes, directions, cigars, the temporary storage, the words
    const FmAlignPlan none = fm_align_plan(0, 0, 0, 0, 0, plenty);
    expect(none.status == FmStatus::Ok && none.scratch_bytes == (3 + 1 + 5 + 1 + 1 + 1 + 1) * 256, "nothing");
    // 5000 alignments of 4000 items, 300000 direction words in global memory, 1500000 CIGAR entries
    const FmAlignPlan p = fm_align_plan(4000, 5000, 300000, 1500000, 9000, plenty);
    expect(p.items == 4000 && p.alignments == 5000 && p.item_bytes == 4000 * 8 + 4001 * 8 + 4000 * 8, "item_bytes");
    expect(p.task_bytes == 5000 * 80 && p.size_bytes == 3 * 5000 * 8 + 2 * 5001 * 8, "alignment_bytes");
    expect(p.direction_bytes == 300000 * 4 && p.cigar_bytes == 1500000 * 4 && p.temp_bytes == 9000 && p.words_bytes == 256, "direction_cigar_temp_words");
    expect(p.scratch_bytes == p.item_bytes + p.task_bytes + p.size_bytes + p.direction_bytes + p.cigar_bytes + p.temp_bytes + p.words_bytes &&
               p.scratch_bytes == 24 * 4000 + 8 + 120 * 5000 + 16 + 4 * 300000 + 4 * 1500000 + 9000 + 256,
           "scratch_is_the_sum");
    // a few: the small buffers stay at the least size
    const FmAlignPlan few = fm_align_plan(2, 3, 0, 10, 0, plenty);
    expect(few.item_bytes == 3 * 256 && few.task_bytes == 256 && few.size_bytes == 5 * 256 && few.direction_bytes == 256 && few.cigar_bytes == 256, "few");
    // free memory: exactly the scratch is served, one byte short is refused with the bytes needed
    expect(fm_align_plan(4000, 5000, 300000, 1500000, 9000, p.scratch_bytes).status == FmStatus::Ok, "capacity_exact_fit");
    const FmAlignPlan shortfall = fm_align_plan(4000, 5000, 300000, 1500000, 9000, p.scratch_bytes - 1);
    expect(shortfall.status == FmStatus::Capacity && shortfall.message.find(std::to_string(p.scratch_bytes)) != std::string::npos &&
               shortfall.message.find(std::to_string(p.scratch_bytes - 1)) != std::string::npos,
           "capacity_one_byte_short");
    // 2^31 alignments are refused whatever the memory, 2^31 - 1 are planned
    const FmAlignPlan many = fm_align_plan(1, uint64_t(1) << 31, 0, 0, 0, 0);
    expect(many.status == FmStatus::Unsupported && many.message.find("2^31") != std::string::npos, "alignments_refused_before_memory");
    expect(fm_align_plan(1, (uint64_t(1) << 31) - 1, 0, 0, 0, plenty).status == FmStatus::Ok && fm_align_plan(1, (uint64_t(1) << 31) - 1, 0, 0, 0, 0).status == FmStatus::Capacity,
           "most_alignments");
    std::printf("%s\n", failures == 0 ? "done" : "failed");
    return failures == 0 ? 0 : 1;
}
