// merge.hpp -- GBWT merging on the device (merge.hip): the record stream of the sequences of two indexes, a's then b's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "build.hpp"
#include "device_index.hpp"

namespace gbwt_hip {

// Bodies of more than this many visits are filled by a workgroup, shorter ones by one lane
constexpr uint32_t MERGE_LONG_RECORD = 64;

// An input as the kernels read it: the record bytes, starts and endmarker every handle keeps, and the header
struct MergeInput {
    DeviceIndex ix;
    uint64_t sequences, visits, alphabet_offset, alphabet_size;
};

struct MergeWalk {
    uint32_t walked_input = 0;             // 0 = a, 1 = b
    uint64_t walked_sequences = 0, walked_steps = 0;
    float walk_ms = 0, decode_ms = 0, interleave_ms = 0;
};

// The records of the merged index by insertion: both inputs bidirectional, at least one visit in the two together (an input without
// visits has the endmarker's record alone), sizes within the widths of the construction (build.hpp).  out.sequences ..
// out.alphabet_size are the caller's; data, starts, peak_scratch, edges_ms and encode_ms are filled.  All scratch is given back before
// it returns.  Throws HipError.
void merge_records_on_device(const MergeInput &a, const MergeInput &b, BuildOutput &out, MergeWalk &walk, hipStream_t s);

// Two CSRs in HBM behind one another (the rows of two extractions): offsets[na + nb + 1], nodes[ta + tb]
void merge_concat_rows(const uint64_t *off_a, const uint32_t *nodes_a, uint64_t na, uint64_t ta, const uint64_t *off_b, const uint32_t *nodes_b, uint64_t nb, uint64_t tb,
                       uint64_t *offsets, uint32_t *nodes, hipStream_t s);

}  // namespace gbwt_hip
