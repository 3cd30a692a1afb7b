// sa_plan.cpp -- csrc/sa_plan.hpp on the host (tests/test_sa_cpu.py builds it with ASan + UBSan): widths, scratch per phase, the peak and
// the two refusals, with the arithmetic that gives the expected values written out.
#include <cstdio>
#include <string>

#include "sa_plan.hpp"

using namespace gbwt_hip;

static int failures = 0;
static void expect(bool ok, const char *name) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
    if (!ok) failures++;
}

int main() {
    const uint64_t plenty = ~uint64_t(0);
    // an empty text: served, nothing held
    const SaPlan none = sa_plan(0, 0, 0);
    expect(none.status == SaStatus::Ok && none.peak_bytes == 0 && none.rank_bits == 0, "n_0_succeeds_without_memory");
    // the widths: a rank is 0 .. n, a round's key two ranks, the first key a whole word
    const SaPlan one = sa_plan(1, 0, plenty);
    expect(one.status == SaStatus::Ok && one.rank_bits == 1 && one.key_bits == 2 && one.first_key_bits == 64, "widths_n_1");
    const SaPlan m3 = sa_plan(3000060, 0, plenty);
    expect(m3.rank_bits == 22 && m3.key_bits == 44, "widths_n_3000060");                   // 2^21 = 2 097 152 <= n < 2^22
    // a small text: every buffer is the smallest buffer; 13 of them (rank, sa, 2 keys, 2 positions, 2 slots, dense, picked, flag, temp, words)
    expect(one.peak_bytes == 13 * SA_MIN_BUFFER && one.settled_bytes == 2 * SA_MIN_BUFFER && one.sort_bytes == 4 * SA_MIN_BUFFER && one.round_bytes == 7 * SA_MIN_BUFFER,
           "small_text_smallest_buffers");
    // 49 bytes per position, the temporary storage and the counters
    const uint64_t n = 1000000, temp = 123456;
    const SaPlan p = sa_plan(n, temp, plenty);
    expect(p.settled_bytes == 8 * n && p.sort_bytes == 24 * n && p.round_bytes == 17 * n + temp + SA_MIN_BUFFER, "bytes_per_phase");
    expect(p.peak_bytes == 49 * n + temp + SA_MIN_BUFFER && p.peak_bytes == p.settled_bytes + p.sort_bytes + p.round_bytes, "peak_is_49_bytes_per_position");
    // free memory: exactly the peak is served, one byte short is refused with the bytes needed, and nothing aborts
    expect(sa_plan(n, temp, p.peak_bytes).status == SaStatus::Ok, "capacity_exact_fit");
    const SaPlan shortfall = sa_plan(n, temp, p.peak_bytes - 1);
    expect(shortfall.status == SaStatus::Capacity && shortfall.message.find(std::to_string(p.peak_bytes)) != std::string::npos &&
               shortfall.message.find(std::to_string(p.peak_bytes - 1)) != std::string::npos,
           "capacity_one_byte_short");
    // the width: 2^32 - 2 positions are the last served, 2^32 - 1 the first refused, whatever memory there is
    const SaPlan last = sa_plan(0xFFFFFFFEull, 0, plenty);
    expect(last.status == SaStatus::Ok && last.rank_bits == 32 && last.key_bits == 64 && last.peak_bytes == 49 * 0xFFFFFFFEull + 2 * SA_MIN_BUFFER, "width_last_served");
    const SaPlan first = sa_plan(0xFFFFFFFFull, 0, plenty);
    expect(first.status == SaStatus::Unsupported && first.message.find("2^32 - 2") != std::string::npos && first.message.find("4294967295") != std::string::npos, "width_first_refused");
    expect(sa_plan(0xFFFFFFFFull, 0, 0).status == SaStatus::Unsupported && sa_plan(~uint64_t(0), 0, plenty).status == SaStatus::Unsupported, "width_refused_before_memory");
    expect(sa_plan(0xFFFFFFFEull, 0, 0).status == SaStatus::Capacity, "width_last_served_still_needs_memory");
    std::printf("%s\n", failures == 0 ? "done" : "failed");
    return failures == 0 ? 0 : 1;
}
