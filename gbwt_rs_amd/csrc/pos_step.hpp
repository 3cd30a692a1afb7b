// pos_step.hpp -- one LF step that carries the in-record offset, Pos{node, offset} -> Pos (the walks of refpos.hip and locate.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "lf_device.hpp"

namespace gbwt_hip {

// GBWT::forward (src/gbwt.rs:222-229) for the lane's position.  FAST: the step of k_forward (query_kernels.hip) on the raw descriptors --
// one rank block on an outdegree-2 record, one LF-table entry where there is a table; everything else decodes the record bytes.
template <bool FAST>
__device__ __forceinline__ bool pos_step(const DeviceIndex &ix, uint64_t &node, uint64_t &offset) {
    uint64_t to_node = 0, to_offset = 0;
    bool ok = false;
    if (FAST) {
        RawDesc d;
        uint64_t rec;
        if (!load_raw_desc(ix, node, d, rec)) return false;
        const uint32_t cls = desc_class(d.B.z);
        if (cls != 0) {
            if (offset >= d.B.w) return false;
            const uint32_t i = static_cast<uint32_t>(offset);
            uint32_t value = 0, rank = i;
            if (cls == 2) {
                const uint4 K = ix.blocks[d.C.z + (i >> RANK_BLOCK_SHIFT)];
                const uint64_t bits = (static_cast<uint64_t>(K.y) << 32) | K.x;
                value = static_cast<uint32_t>(bits >> (i & 63u)) & 1u;
                const uint32_t ones = K.z + __popcll(bits & ((uint64_t(1) << (i & 63u)) - 1));
                rank = value ? ones : i - ones;
            }
            to_node = value ? d.A.z : d.A.x;
            to_offset = static_cast<uint64_t>(value ? d.A.w : d.A.y) + rank;
            ok = to_node != 0;
        } else if (d.C.w == 1u) {
            if (offset >= d.C.y) return false;
            const uint4 e = ix.tables[static_cast<uint64_t>(d.C.z) + offset];
            to_node = e.x; to_offset = e.y;
            ok = e.x != 0;
        } else {                                     // a record without a table: its bytes, found through the descriptor (dev_follow, query_kernels.hip)
            const uint64_t start = desc_start(d.B.x, d.B.z);
            ByteCursor c(ix.data, start, start + d.B.y);
            uint64_t sigma;
            ok = c.varint(sigma) && sigma != 0 && record_lf(c, sigma, offset, to_node, to_offset);
        }
    } else ok = gbwt_forward(ix, node, offset, to_node, to_offset);
    node = to_node; offset = to_offset;
    return ok;
}

}  // namespace gbwt_hip
