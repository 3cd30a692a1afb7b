// launch_scan and launch_block_scan (csrc/scan.hpp) ON THE DEVICE, against host prefix sums: empty scans, one piece, piece boundaries, a last
// partial piece.  Inputs below 2^40, so the sums pass 2^32 and never wrap.  Checked: exact sums, out[0] == 0, the input unchanged, a guard word
// behind out[n] untouched, with temp storage of exactly scan_temp_bytes(n, piece).  Built with csrc/scan.hip and run by tests/test_gpu_scan.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <random>
#include <vector>

#include "scan.hpp"

using namespace gbwt_hip;

namespace {

constexpr uint64_t GUARD = 0xA5A5A5A5DEADBEEFull;

#define CHECK(call) do { if ((call) != hipSuccess) { std::printf("%s failed: %s\n", #call, hipGetErrorString(hipGetLastError())); return false; } } while (0)

bool check_scan(uint64_t n, uint64_t piece, std::mt19937_64 &rng) {
    std::vector<uint64_t> in(n), want(n + 1, 0), back(n), out(n + 2);
    for (uint64_t i = 0; i < n; i++) { in[i] = rng() & ((uint64_t(1) << 40) - 1); want[i + 1] = want[i] + in[i]; }
    const size_t temp_bytes = scan_temp_bytes(n, piece);
    if (temp_bytes == 0) { std::printf("scan_temp_bytes(%llu, %llu) is 0\n", (unsigned long long)n, (unsigned long long)piece); return false; }
    uint64_t *d_in = nullptr, *d_out = nullptr;
    void *d_temp = nullptr;
    CHECK(hipMalloc(&d_in, (n + 1) * 8));
    CHECK(hipMalloc(&d_out, (n + 2) * 8));
    CHECK(hipMalloc(&d_temp, temp_bytes));
    if (n) CHECK(hipMemcpy(d_in, in.data(), n * 8, hipMemcpyHostToDevice));
    std::vector<uint64_t> fill(n + 2, GUARD);
    CHECK(hipMemcpy(d_out, fill.data(), (n + 2) * 8, hipMemcpyHostToDevice));
    launch_scan(d_in, d_out, n, d_temp, temp_bytes, nullptr, piece);
    CHECK(hipDeviceSynchronize());
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(out.data(), d_out, (n + 2) * 8, hipMemcpyDeviceToHost));
    if (n) CHECK(hipMemcpy(back.data(), d_in, n * 8, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in)); CHECK(hipFree(d_out)); CHECK(hipFree(d_temp));
    if (out[0] != 0) { std::printf("out[0] = %llu\n", (unsigned long long)out[0]); return false; }
    for (uint64_t i = 0; i <= n; i++)
        if (out[i] != want[i]) { std::printf("out[%llu] = %llu, expected %llu\n", (unsigned long long)i, (unsigned long long)out[i], (unsigned long long)want[i]); return false; }
    if (out[n + 1] != GUARD) { std::printf("the word behind out[n] was written\n"); return false; }
    if (back != in) { std::printf("the input was modified\n"); return false; }
    return true;
}

bool check_block_scan(uint64_t n, std::mt19937_64 &rng) {
    std::vector<uint32_t> in(n), want(n, 0), out(n + 1), back(n);
    for (uint64_t i = 0; i < n; i++) { in[i] = static_cast<uint32_t>(rng() % 1000); if (i + 1 < n) want[i + 1] = want[i] + in[i]; }
    size_t temp_bytes = block_scan_temp_bytes(n);
    uint32_t *d_in = nullptr, *d_out = nullptr;
    void *d_temp = nullptr;
    CHECK(hipMalloc(&d_in, n * 4));
    CHECK(hipMalloc(&d_out, (n + 1) * 4));
    CHECK(hipMalloc(&d_temp, temp_bytes ? temp_bytes : 16));
    CHECK(hipMemcpy(d_in, in.data(), n * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xA5, (n + 1) * 4));
    launch_block_scan(d_in, d_out, n, d_temp, temp_bytes, nullptr);
    CHECK(hipDeviceSynchronize());
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(out.data(), d_out, (n + 1) * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(back.data(), d_in, n * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in)); CHECK(hipFree(d_out)); CHECK(hipFree(d_temp));
    for (uint64_t i = 0; i < n; i++)
        if (out[i] != want[i]) { std::printf("block out[%llu] = %u, expected %u\n", (unsigned long long)i, out[i], want[i]); return false; }
    if (out[n] != 0xA5A5A5A5u) { std::printf("the word behind the block scan's output was written\n"); return false; }
    if (back != in) { std::printf("the block scan's input was modified\n"); return false; }
    return true;
}

}  // namespace

int main() {
    std::mt19937_64 rng(11);
    for (uint64_t piece : {uint64_t(1024), uint64_t(4096), SCAN_PIECE}) {
        const uint64_t p = piece == SCAN_PIECE ? 4096 : piece;       // the default piece: the same n list, all of it one piece
        for (uint64_t n : {uint64_t(0), uint64_t(1), p - 1, p, p + 1, 2 * p, 2 * p + 1, 3 * p + 17}) {
            if (!check_scan(n, piece, rng)) { std::printf("FAILED scan n=%llu piece=%llu\n", (unsigned long long)n, (unsigned long long)piece); return 1; }
            std::printf("ok scan n=%llu piece=%llu\n", (unsigned long long)n, (unsigned long long)piece);
        }
    }
    for (uint64_t n : {uint64_t(1), uint64_t(1025)}) {
        if (!check_block_scan(n, rng)) { std::printf("FAILED block_scan n=%llu\n", (unsigned long long)n); return 1; }
        std::printf("ok block_scan n=%llu\n", (unsigned long long)n);
    }
    std::printf("done\n");
    return 0;
}
