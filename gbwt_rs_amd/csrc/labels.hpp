// labels.hpp -- the node labels of a handle as the kernels see them (sequences.hip, tags.hip, capi_topology.hip, capi_refpos.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

struct gbwt_hip_index;

namespace gbwt_hip {

// The labels of a handle as the kernels see them (sequences.hip, tags.hip): node v (GBWT-encoded, 2 id + o) has label bytes[off[s] .. off[s + 1])
// with s = (v & ~1 - first_node) / 2 (GBZ::graph_node_to_sequence, src/gbz.rs:246-255); a node outside [first_node, first_node + 2 n) has none.
struct Labels { const uint8_t *bytes; const uint64_t *off; uint64_t n; uint32_t first_node; };

__device__ __forceinline__ void label_of(const Labels &L, uint32_t node, uint64_t &lo, uint64_t &hi) {
    const uint32_t fwd = node & ~1u;
    const uint64_t s = (static_cast<uint64_t>(fwd) - L.first_node) / 2;
    if (fwd < L.first_node || s >= L.n) { lo = 0; hi = 0; return; }
    lo = L.off[s]; hi = L.off[s + 1];
}

// sequences.hip: the labels of a handle in HBM (made by the first request that needs them), and the test every entry point for bases
// (capi_sequences.hip), tags (capi_tags.hip) and the suffix array of paths (capi_suffix_array.hip) starts with (InvalidData for a bare GBWT
// or a handle without GBWT_HIP_OPEN_EXTRACT)
Labels labels_of(const gbwt_hip_index *ix);
void ensure_labels(const gbwt_hip_index *ix);
void require_bases_capable(const gbwt_hip_index *ix);

}  // namespace gbwt_hip
