// build.hpp -- GBWT construction on the device (build.hip): the record stream of a set of paths that lie in HBM as a CSR.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gbwt_hip.h"
#include "host_index.hpp"

namespace gbwt_hip {

// Widths of the construction (include/gbwt_hip.h, "construction"): a slot of the text is a visit or the start of a sequence, and slots,
// ranks and offsets inside a record are u32
constexpr uint64_t BUILD_MAX_SLOTS = 0xFFFFFFFFull;      // visits + sequences
constexpr uint64_t BUILD_MAX_RECORDS = uint64_t(1) << 30;   // what an open takes (bits 30-31 of a record word carry flags)

struct BuildInput {
    const uint64_t *d_offsets;    // [n_paths + 1], in HBM
    const uint32_t *d_nodes;      // [visits of the paths], in HBM; only read
    uint64_t n_paths, path_visits;
    bool bidirectional;
    uint64_t min_node, max_node;  // over the SEQUENCES (with the flipped nodes of the reverse ones); unused without visits
};

struct BuildOutput {
    Bytes data;                   // the record stream
    Words starts;                 // [records]
    uint64_t sequences = 0, visits = 0, records = 0, alphabet_offset = 0, alphabet_size = 1;
    uint32_t rounds = 0;          // doubling rounds of the ranking
    uint64_t peak_scratch = 0;    // most bytes of HBM the construction held at once (without the caller's rows)
    float expand_ms = 0, rank_ms = 0, edges_ms = 0, encode_ms = 0;
};

// The records of the index of the paths, computed on stream `s` of the current device and copied to the host; all
// scratch is given back before it returns.  Needs at least one visit (the caller writes the index of a set without visits itself)
// and sizes within the limits above.  Throws HipError.
void build_records_on_device(const BuildInput &in, BuildOutput &out, hipStream_t s);

// min and max of n > 0 nodes in HBM (the caller of a device-resident input checks and sizes with them)
void build_node_range(const uint32_t *d_nodes, uint64_t n, uint32_t &min_node, uint32_t &max_node, hipStream_t s);

// capi_build.hip, shared with the construction from GFA (capi_gfa_build.hip): the widths of the construction as statuses (the message
// in the thread's error slot), and the records of a set of paths without visits
gbwt_hip_status check_build_sizes(uint64_t n_paths, uint64_t path_visits, int bidirectional);
gbwt_hip_status check_build_range(uint64_t min_node, uint64_t max_node);
void build_without_visits(uint64_t sequences, BuildOutput &out);

}  // namespace gbwt_hip
