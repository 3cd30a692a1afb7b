// build.hpp -- GBWT construction on the device (build.hip): the record stream of a set of paths that lie in HBM as a CSR.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <memory>

#include "../../include/gbwt_hip.h"
#include "capi_internal.hpp"
#include "counted_buffer.hpp"
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

// The sorted slots as record bodies, on their way to bytes (build.hip: encode_sorted_bodies).  The edge lists are in hand when the
// offsets are asked for: edge[e] = (node of the record << 32) | successor, sorted; record r owns [edge_first[r], edge_first[r + 1]) and the
// positions from visit_first[r] on; edge_offset is zeroed.  `launch` starts the kernel that fills edge_offset on the stream; `release`
// (may be empty) gives back what only that kernel read, once it is done.
struct BodyEdges {
    const uint64_t *edge;
    uint64_t edges;
    const uint32_t *edge_first, *visit_first;
    uint32_t *edge_offset;
};
struct BodyOffsets {
    std::function<void(const BodyEdges &)> launch;
    std::function<void()> release;
};

// The records of the index of the paths, computed on stream `s` of the current device and copied to the host; all
// scratch is given back before it returns.  Needs at least one visit (the caller writes the index of a set without visits itself)
// and sizes within the limits above.  Throws HipError.
void build_records_on_device(const BuildInput &in, BuildOutput &out, hipStream_t s);

// build.hip: from the sorted bodies to the record stream in out.data / out.starts (and out.edges_ms, counted from `begin`, an event
// the caller has recorded on s, and out.encode_ms).  rec[i]: the node of position i's record (0: the endmarker's), succ[i]: its
// successor; both are given back on the way.  temp: scratch of the library calls, any size, grown as needed.
void encode_sorted_bodies(CountedBuf &rec, CountedBuf &succ, uint64_t slots, uint64_t records, uint64_t alphabet_offset, const BodyOffsets &offsets, CountedScratch &sc, CountedBuf &temp,
                          BuildOutput &out, hipEvent_t begin, hipStream_t s);

// min and max of n > 0 nodes in HBM (the caller of a device-resident input checks and sizes with them)
void build_node_range(const uint32_t *d_nodes, uint64_t n, uint32_t &min_node, uint32_t &max_node, hipStream_t s);

// capi_build.hip, shared with the construction from GFA (capi_gfa_build.hip): the widths of the construction as statuses (the message
// in the thread's error slot), and the records of a set of paths without visits
gbwt_hip_status check_build_sizes(uint64_t n_paths, uint64_t path_visits, int bidirectional);
gbwt_hip_status check_build_range(uint64_t min_node, uint64_t max_node);
void build_without_visits(uint64_t sequences, BuildOutput &out);

// THE ROAD FROM RECORDS TO A HANDLE, the same for every maker (construction, from GFA, merge, removal): the new handle
// (new_handle) with its host image filled from the records (index_from_records).  The caller decorates the image -- metadata, tags, graph
// (host_index.hpp: adopt_metadata) -- and hands it to open_host_index.
std::unique_ptr<gbwt_hip_index> handle_from_build(const BuildOutput &o, bool bidirectional, int device, uint32_t flags);

// What gbwt_hip_build_info, gbwt_hip_merge_info and gbwt_hip_remove_info say about the records, under the same names
template <class Info>
static void fill_build_counters(Info &m, const BuildOutput &o) {
    m.visits = o.visits; m.sequences = o.sequences; m.records = o.records; m.data_bytes = o.data.size(); m.peak_scratch_bytes = o.peak_scratch;
    m.rounds = o.rounds; m.edges_ms = o.edges_ms; m.encode_ms = o.encode_ms;
}
// ... and the whole of a gbwt_hip_build_info but open_ms, which the caller knows behind the open
inline gbwt_hip_build_info build_info_of(const BuildOutput &o) {
    gbwt_hip_build_info b{};
    fill_build_counters(b, o);
    b.built = 1; b.expand_ms = o.expand_ms; b.rank_ms = o.rank_ms;
    return b;
}

}  // namespace gbwt_hip
