// build_codec.hpp -- the encoder side of a GBWT record, shared by the construction kernels (build.hip), the host path of
// capi_build.hip and a stand-alone host test (tests/cpp/build_codec.cpp): one text for both, as gfa_tokens.hpp is.
//
// A record is  varint(sigma)  (successor delta, offset) varint pairs  runs  (BWTBuilder::append, src/bwt.rs:241-253):
//   varint   ByteCode, src/support.rs:1063-1070: 7 bits per byte, low bits first, the high bit says "more"
//   run      RLE, src/support.rs:1238-1248: for sigma < 255, threshold = 256 / sigma, one byte value + sigma * (len - 1) while
//            len < threshold, else the byte value + sigma * (threshold - 1) and varint(len - threshold); for sigma >= 255
//            varint(value), varint(len - 1)
// Every size function returns what its write function writes.  A writer takes the place of the first byte and returns the place
// behind the last one; it stores byte by byte (plain stores: one lane per item on the device).
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GBWT_BUILD_HD __host__ __device__ inline
#else
#define GBWT_BUILD_HD inline
#endif

namespace gbwt_hip {
namespace build_codec {

GBWT_BUILD_HD uint32_t varint_size(uint64_t v) {
    uint32_t n = 1;
    while (v > 0x7F) { v >>= 7; n++; }
    return n;
}

GBWT_BUILD_HD uint8_t *write_varint(uint8_t *p, uint64_t v) {
    while (v > 0x7F) { *p++ = static_cast<uint8_t>((v & 0x7F) | 0x80); v >>= 7; }
    *p++ = static_cast<uint8_t>(v);
    return p;
}

// a run of `len` >= 1 copies of edge rank `value` < sigma in a record of outdegree sigma >= 1
GBWT_BUILD_HD uint32_t run_size(uint64_t sigma, uint64_t value, uint64_t len) {
    if (sigma >= 255) return varint_size(value) + varint_size(len - 1);
    const uint64_t threshold = 256 / sigma;
    return len < threshold ? 1u : 1u + varint_size(len - threshold);
}

GBWT_BUILD_HD uint8_t *write_run(uint8_t *p, uint64_t sigma, uint64_t value, uint64_t len) {
    if (sigma >= 255) return write_varint(write_varint(p, value), len - 1);
    const uint64_t threshold = 256 / sigma;
    if (len < threshold) { *p++ = static_cast<uint8_t>(value + sigma * (len - 1)); return p; }
    *p++ = static_cast<uint8_t>(value + sigma * (threshold - 1));
    return write_varint(p, len - threshold);
}

// the head of a record: its outdegree (a record nobody visits is the one byte 0)
GBWT_BUILD_HD uint32_t header_size(uint64_t sigma) { return varint_size(sigma); }
GBWT_BUILD_HD uint8_t *write_header(uint8_t *p, uint64_t sigma) { return write_varint(p, sigma); }

// one entry of the edge list: the successor as its distance from the one before it (from 0 for the first), and the edge's offset
GBWT_BUILD_HD uint32_t edge_size(uint64_t delta, uint64_t offset) { return varint_size(delta) + varint_size(offset); }
GBWT_BUILD_HD uint8_t *write_edge(uint8_t *p, uint64_t delta, uint64_t offset) { return write_varint(write_varint(p, delta), offset); }

}  // namespace build_codec
}  // namespace gbwt_hip
