// The encoder side of a GBWT record (csrc/build_codec.hpp, shared with the construction kernels) compiled for the host: every size function
// against what its write function writes, and the bytes as hex for tests/test_build_capi_cpu.py, which compares them with the oracle's
// ByteCode / RLE encoders.  Each case is written into the middle of a guarded buffer: a writer that leaves its bytes is caught here,
// one that leaves the buffer by the sanitizers this program is built with.
//   varint <value> <size> <hex>
//   run <sigma> <value> <len> <size> <hex>
//   header <sigma> <size> <hex>
//   edge <delta> <offset> <size> <hex>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "build_codec.hpp"

namespace bc = gbwt_hip::build_codec;

static int failures = 0;

template <class W>
static void emit(const char *what, uint32_t size, W write) {
    constexpr size_t GUARD = 16;
    std::vector<uint8_t> buf(GUARD + size + GUARD, 0xA5);
    uint8_t *end = write(buf.data() + GUARD);
    if (end != buf.data() + GUARD + size) { std::printf("FAIL %s: size function says %u, writer wrote %td\n", what, size, end - (buf.data() + GUARD)); failures++; }
    for (size_t k = 0; k < GUARD; k++)
        if (buf[k] != 0xA5 || buf[GUARD + size + k] != 0xA5) { std::printf("FAIL %s: a byte outside the item was written\n", what); failures++; break; }
    std::printf("%s %u ", what, size);
    for (uint32_t k = 0; k < size; k++) std::printf("%02x", buf[GUARD + k]);
    std::printf("\n");
}

int main() {
    char what[128];
    const uint64_t varints[] = {0, 127, 128, 16383, 16384, 0xFFFFFFFFull};
    for (uint64_t v : varints) {
        std::snprintf(what, sizeof(what), "varint %" PRIu64, v);
        emit(what, bc::varint_size(v), [&](uint8_t *p) { return bc::write_varint(p, v); });
        std::snprintf(what, sizeof(what), "header %" PRIu64, v);
        emit(what, bc::header_size(v), [&](uint8_t *p) { return bc::write_header(p, v); });
        for (uint64_t o : varints) {
            std::snprintf(what, sizeof(what), "edge %" PRIu64 " %" PRIu64, v, o);
            emit(what, bc::edge_size(v, o), [&](uint8_t *p) { return bc::write_edge(p, v, o); });
        }
    }
    const uint64_t sigmas[] = {1, 2, 85, 86, 128, 129, 254, 255, 300};
    for (uint64_t sigma : sigmas) {
        const uint64_t threshold = 256 / sigma;      // 1 for 255, 0 for 300: the two-varint form has none, the lengths below still vary
        const uint64_t lens[] = {1, threshold - 1, threshold, threshold + 127, threshold + 128, 100000};
        for (uint64_t len : lens) {
            if (len == 0 || len > 100000) continue;  // (threshold - 1 of a threshold below 2)
            const uint64_t values[] = {0, sigma / 2, sigma - 1};
            for (uint64_t value : values) {
                std::snprintf(what, sizeof(what), "run %" PRIu64 " %" PRIu64 " %" PRIu64, sigma, value, len);
                emit(what, bc::run_size(sigma, value, len), [&](uint8_t *p) { return bc::write_run(p, sigma, value, len); });
            }
        }
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("done\n");
    return 0;
}
