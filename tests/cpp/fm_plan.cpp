// fm_plan.cpp -- csrc/fm_plan.hpp on the host (tests/test_fm_cpu.py builds it with ASan + UBSan): the sizes of both layouts, the refusal
// above 2^32 - 2 positions and the capacity arithmetic, with the arithmetic that gives the expected values written out.
#include <cstdio>
#include <string>

#include "fm_plan.hpp"

using namespace gbwt_hip;

static int failures = 0;
static void expect(bool ok, const char *name) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
    if (!ok) failures++;
}

int main() {
    const uint64_t plenty = ~uint64_t(0);
    // an empty text: one row, one line, the tables; no suffix array, no scratch but the histogram and the words
    const FmPlan none = fm_plan(0, 0, false, true, 0, plenty);
    expect(none.status == FmStatus::Ok && none.rows == 1 && none.blocks == 1 && none.packed && none.sa_bytes == 0 && none.index_bytes == SA_MIN_BUFFER + FM_TABLE_BYTES &&
               none.scratch_bytes == FM_HISTOGRAM_BYTES + SA_MIN_BUFFER,
           "n_0");
    expect(FM_TABLE_BYTES == 1536 && FM_HISTOGRAM_BYTES == 2048, "table_and_histogram_bytes");
    // packed: n = 959 gives 960 rows = 10 whole blocks and one more for rank(c, rows): 11 lines of 128 bytes
    const FmPlan p = fm_plan(959, 6, false, false, 1000, plenty);
    expect(p.packed && p.block_rows == 96 && p.rows == 960 && p.blocks == 11 && p.lines_bytes == 11 * 128 && p.counts_bytes == 0 && p.sa_bytes == 959 * 4, "packed_sizes");
    expect(p.index_bytes == 11 * 128 + 1536 + 959 * 4 && p.block_count_bytes == 11 * 6 * 4 && p.scratch_bytes == 2048 + 256 + 2 * 11 * 6 * 4 + 1000 && p.peak_bytes == p.index_bytes + p.scratch_bytes,
           "packed_index_and_scratch");
    expect(fm_plan(958, 6, false, false, 0, plenty).blocks == 10 && fm_plan(95, 8, false, false, 0, plenty).blocks == 2 && fm_plan(94, 8, false, false, 0, plenty).blocks == 1, "packed_block_edges");
    // count-only: no suffix array; a build that makes the suffix array itself: 8 bytes per position of scratch
    const FmPlan c = fm_plan(959, 6, true, true, 1000, plenty);
    expect(c.sa_bytes == 0 && c.index_bytes == 11 * 128 + 1536 && c.sa64_bytes == 959 * 8 && c.scratch_bytes == p.scratch_bytes + 959 * 8, "count_only_and_own_suffix_array");
    // plain: sigma = 9 is the first; 1023 positions = 1024 rows = 4 blocks and one more; counts 5 * sigma words
    const FmPlan q = fm_plan(1023, 256, false, false, 0, plenty);
    expect(!q.packed && q.block_rows == 256 && q.blocks == 5 && q.lines_bytes == 5 * 256 && q.counts_bytes == 5 * 256 * 4 && q.index_bytes == 5 * 256 + 5 * 1024 + 1536 + 1023 * 4, "plain_sizes");
    expect(!fm_plan(100, 9, false, false, 0, plenty).packed && fm_plan(100, 8, false, false, 0, plenty).packed, "plain_from_sigma_9");
    // bytes per position of a long text: 128 / 96 packed, 1 + sigma / 64 plain, and 4 for the suffix array
    const uint64_t n = 96000000 - 1;
    const FmPlan big = fm_plan(n, 6, false, false, 0, plenty);
    expect(big.lines_bytes == (n + 1) / 96 * 128 + 128 && big.sa_bytes == 4 * n, "packed_bytes_per_position");
    const uint64_t n2 = 25600000 - 1;
    const FmPlan big2 = fm_plan(n2, 256, true, false, 0, plenty);
    expect(big2.lines_bytes == n2 + 1 + 256 && big2.counts_bytes == ((n2 + 1) / 256 + 1) * 1024, "plain_bytes_per_position");
    // free memory: exactly the peak is served, one byte short is refused with the bytes needed
    expect(fm_plan(959, 6, false, false, 1000, p.peak_bytes).status == FmStatus::Ok, "capacity_exact_fit");
    const FmPlan shortfall = fm_plan(959, 6, false, false, 1000, p.peak_bytes - 1);
    expect(shortfall.status == FmStatus::Capacity && shortfall.message.find(std::to_string(p.peak_bytes)) != std::string::npos &&
               shortfall.message.find(std::to_string(p.peak_bytes - 1)) != std::string::npos,
           "capacity_one_byte_short");
    // the width: 2^32 - 2 positions are the last served, 2^32 - 1 the first refused, whatever memory there is
    const FmPlan last = fm_plan(0xFFFFFFFEull, 6, false, false, 0, plenty);
    expect(last.status == FmStatus::Ok && last.sa_bytes == 4 * 0xFFFFFFFEull && last.rows == 0xFFFFFFFFull, "width_last_served");
    const FmPlan first = fm_plan(0xFFFFFFFFull, 6, false, false, 0, plenty);
    expect(first.status == FmStatus::Unsupported && first.message.find("2^32 - 2") != std::string::npos && first.message.find("4294967295") != std::string::npos, "width_first_refused");
    expect(fm_plan(0xFFFFFFFFull, 6, true, false, 0, 0).status == FmStatus::Unsupported && fm_check_width(~uint64_t(0)).status == FmStatus::Unsupported &&
               fm_check_width(0xFFFFFFFEull).status == FmStatus::Ok,
           "width_refused_before_memory");
    expect(fm_plan(0xFFFFFFFEull, 6, false, false, 0, 0).status == FmStatus::Capacity, "width_last_served_still_needs_memory");
    std::printf("%s\n", failures == 0 ? "done" : "failed");
    return failures == 0 ? 0 : 1;
}
