// remove.hpp -- path removal on the device (remove.hip): the record stream of an index without some of its sequences.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "build.hpp"
#include "merge.hpp"

namespace gbwt_hip {

// walk_ms: clearing the marks, the ids to the device, the marking walk; compact_ms: the prefix sum, its total to the host, the scatter and
// the min / max of the new alphabet (gbwt_hip_remove_info)
struct RemoveWalk {
    uint64_t removed_sequences = 0, removed_steps = 0;
    float walk_ms = 0, decode_ms = 0, compact_ms = 0;
};

// The records of the index of the sequences of `in` that are not among removed[0, n) (sequence ids, distinct, below in.sequences; on the
// host), in their old order: marks, compaction and the construction's edge, size and fill phases (build.hpp).  Bidirectional or not: the
// caller names both sequences of a path.  Every field of `out` is filled -- sequences, visits, the alphabet of the kept sequences,
// records, data, starts, peak_scratch, edges_ms, encode_ms; without a kept visit it is build_without_visits(kept sequences).  All scratch
// is given back before it returns.  The caller has checked the INPUT against the widths of the construction (check_build_sizes): positions
// are u32 here.  Throws HipError, and InvalidData for records that are not consistent (the error word of the kernels).
void remove_records_on_device(const MergeInput &in, const uint64_t *removed, uint64_t n, BuildOutput &out, RemoveWalk &walk, hipStream_t s);

}  // namespace gbwt_hip
