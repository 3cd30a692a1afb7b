// fm_chain_plan.cpp -- csrc/fm_chain_plan.hpp on the host (tests/test_chains_cpu.py builds it with ASan + UBSan): the bytes of the chaining's
// scratch with the arithmetic that gives the expected values written out, the refusal, and the capacity arithmetic.
#include <cstdio>
#include <string>

#include "fm_chain_plan.hpp"

using namespace gbwt_hip;

static int failures = 0;
static void expect(bool ok, const char *name) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
    if (!ok) failures++;
}

int main() {
    const uint64_t plenty = ~uint64_t(0);
    expect(FM_CHAIN_MIN_BUFFER == 256 && FM_CHAIN_WORDS == 4 && FM_CHAIN_TILE == 512 && FM_CHAIN_MAX_HITS == 0x7FFFFFFFull, "constants");
    // nothing to chain: every buffer at its least size -- 3 per item, 4 of the sort, 7 per match, 5 of the peeling, 4 of the rows, the
    // temporary storage, the words
    const FmChainPlan none = fm_chain_plan(0, 0, 0, plenty);
    expect(none.status == FmStatus::Ok && none.scratch_bytes == (3 + 4 + 7 + 5 + 4 + 1 + 1) * 256, "nothing");
    // 100000 hits of 2000 items
    const FmChainPlan p = fm_chain_plan(100000, 2000, 70000, plenty);
    expect(p.hits == 100000 && p.items == 2000 && p.item_bytes == 2000 * 8 + 2 * 2001 * 8, "item_bytes");
    expect(p.sort_bytes == 4 * 100000 * 8 && p.match_bytes == 7 * 100000 * 4 && p.peel_bytes == 100000 + 4 * 100000 * 4 && p.row_bytes == 2 * 100000 * 8 + 2 * 100001 * 8, "hit_bytes");
    expect(p.temp_bytes == 70000 && p.words_bytes == 256, "temp_and_words");
    expect(p.scratch_bytes == p.item_bytes + p.sort_bytes + p.match_bytes + p.peel_bytes + p.row_bytes + p.temp_bytes + p.words_bytes &&
               p.scratch_bytes == 109 * 100000 + 16 + 24 * 2000 + 16 + 70000 + 256,
           "scratch_is_the_sum");
    // few hits: the buffers of bytes and of u32 stay at the least size
    const FmChainPlan few = fm_chain_plan(40, 3, 0, plenty);
    expect(few.item_bytes == 3 * 256 && few.sort_bytes == 4 * 320 && few.match_bytes == 7 * 256 && few.peel_bytes == 5 * 256 && few.row_bytes == 2 * 320 + 2 * 328, "few_hits");
    // free memory: exactly the scratch is served, one byte short is refused with the bytes needed
    expect(fm_chain_plan(100000, 2000, 70000, p.scratch_bytes).status == FmStatus::Ok, "capacity_exact_fit");
    const FmChainPlan shortfall = fm_chain_plan(100000, 2000, 70000, p.scratch_bytes - 1);
    expect(shortfall.status == FmStatus::Capacity && shortfall.message.find(std::to_string(p.scratch_bytes)) != std::string::npos &&
               shortfall.message.find(std::to_string(p.scratch_bytes - 1)) != std::string::npos,
           "capacity_one_byte_short");
    // 2^31 hits are refused whatever the memory, 2^31 - 1 are planned
    const FmChainPlan wide = fm_chain_plan(uint64_t(1) << 31, 1, 0, 0);
    expect(wide.status == FmStatus::Unsupported && wide.message.find("2^31") != std::string::npos, "hits_refused_before_memory");
    expect(fm_chain_plan((uint64_t(1) << 31) - 1, 1, 0, plenty).status == FmStatus::Ok && fm_chain_plan((uint64_t(1) << 31) - 1, 1, 0, 0).status == FmStatus::Capacity, "most_hits");
    std::printf("%s\n", failures == 0 ? "done" : "failed");
    return failures == 0 ? 0 : 1;
}
