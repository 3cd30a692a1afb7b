// merge.hpp -- GBWT merging on the device (merge.hip): the record stream of the sequences of two indexes, a's then b's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "build.hpp"
#include "device_index.hpp"
#include "lf_device.hpp"
#include "merge_meta.hpp"

namespace gbwt_hip {

// Bodies of more than this many visits are filled by a workgroup, shorter ones by one lane
constexpr uint32_t MERGE_LONG_RECORD = 64;

// ---- device helpers over the records of an input, shared by merge.hip and remove.hip ------------------------------------------------------
// In a namespace of their own, which those two files open: no other file that includes this header sees the names.
namespace record_access {

constexpr uint64_t NO_RECORD = ~uint64_t(0);

// entries of a[0, n) that are <= x (a is non-decreasing)
__device__ __forceinline__ uint64_t merge_upper_bound(const uint32_t *a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the record of node v (0: the endmarker), or NO_RECORD
__device__ __forceinline__ uint64_t record_of_node(const DeviceIndex &ix, uint64_t v) {
    if (v == 0) return 0;
    if (v <= ix.alphabet_offset) return NO_RECORD;
    const uint64_t r = v - ix.alphabet_offset;
    return r < ix.n_records ? r : NO_RECORD;
}

__device__ __forceinline__ uint64_t node_of_record(const DeviceIndex &ix, uint64_t r) { return r == 0 ? 0 : r + ix.alphabet_offset; }

// opens record r: the cursor stands behind sigma; false for an empty record
__device__ __forceinline__ bool open_by_record(const DeviceIndex &ix, uint64_t r, ByteCursor &c, uint64_t &sigma) {
    if (r >= ix.n_records) return false;
    uint64_t start, limit;
    record_bounds(ix, r, start, limit);
    if (start >= limit || limit > ix.data_len) return false;
    c = ByteCursor(ix.data, start, limit);
    if (!c.varint(sigma)) return false;
    return sigma != 0;
}

// the stored offset of edge v -> w in X (v, w real nodes); false when X has no such edge
__device__ __forceinline__ bool edge_offset_of(const DeviceIndex &ix, uint64_t v, uint64_t w, uint64_t &offset) {
    ByteCursor c(ix.data, 0, 0);
    uint64_t sigma;
    const uint64_t r = record_of_node(ix, v);
    if (r == NO_RECORD || !open_by_record(ix, r, c, sigma)) return false;
    uint64_t node = 0;
    for (uint64_t e = 0; e < sigma; e++) {
        uint64_t delta, off;
        if (!c.varint(delta) || !c.varint(off)) return false;
        node += delta;
        if (node == w) { offset = off; return true; }
        if (node > w) return false;
    }
    return false;
}

}  // namespace record_access

// A refusal of the host's part (merge_meta.hpp, remove_meta.hpp) as a status; prefix: "merge: " or "remove: "
inline gbwt_hip_status refusal_status(const MergeRefusal &bad, const char *prefix) {
    return fail(bad.kind == MergeRefusal::UNSUPPORTED ? GBWT_HIP_UNSUPPORTED : GBWT_HIP_INVALID_DATA, prefix + bad.what);
}

// An input as the kernels read it: the record bytes, starts and endmarker every handle keeps, and the header
struct MergeInput {
    DeviceIndex ix;
    uint64_t sequences, visits, alphabet_offset, alphabet_size;
};

// first[] (records + 1 entries: the first position of every record, the endmarker's first) and the successor of every position
struct MergeDecoded {
    CountedBuf first, body;
    uint64_t positions = 0;
};

// Lengths, scan and bodies of one input (k_merge_count, k_merge_decode*): also the first phase of a removal (remove.hip).  temp: scratch
// of the library calls, any size, grown as needed.  Throws InvalidData where the records do not hold what the header says.
void merge_decode_bodies(const MergeInput &in, MergeDecoded &d, CountedScratch &sc, CountedBuf &temp, hipStream_t s);

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
