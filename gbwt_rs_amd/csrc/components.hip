// components.hip -- weakly connected components of the graph (GBZ::weakly_connected_components, src/gbz.rs:570-598) from what every handle keeps
// in HBM: the record byte stream, the dense record starts and the decompressed endmarker.
//
// The reference walks the graph with a stack and a union-find (DisjointSets, src/support.rs:1480-1576): every successor and predecessor of a
// node joins the two node ids, whatever the orientations; DisjointSets::extract lists the nodes that exist (GBZ::has_node), the sets in order
// of their smallest node, the nodes ascending inside.  Here one label per NODE SLOT (ComponentGeometry) converges to the smallest slot of its
// component by rounds of
//   k_hook  one lane per record: the edge-list header is decoded from the record bytes (outdegree, then (node delta, offset) pairs,
//           Record::decompress_edges, src/bwt.rs:378-395), and every successor other than the ENDMARKER (EdgeIter::new skips it,
//           src/gbz.rs:834-836) with parent[u] != parent[v] hooks the larger of the two parents under the smaller (atomicMin).  Predecessors
//           need no pass of their own: those of (v, o) are the successors in the record of (v, flip o), which the sweep visits anyway.
//   k_jump  parent[s] = parent[parent[s]], launched until a device flag says that nothing changed: every tree is a star again.
// until a hook pass changes nothing.  A hook may lose against another one on the same parent (the smallest wins) or undo an older link of a
// slot that is no root any more; the edge that made the lost link finds parent[u] != parent[v] in the next hook pass and hooks again.  Every
// change lowers a label, labels never leave their component, and the loop ends when both ends of every edge carry the same label and all
// trees are stars: one star per component, its root -- never larger than a member, and a member itself -- the smallest slot.  Ordering comes
// from kernel boundaries alone: inside a launch a stale label is an older ancestor, which is as good as the newer one; no pass relies on
// seeing what another workgroup of the same launch wrote.
//
// Output shaping (off the hot path): the smallest EXISTING slot of every component (atomicMin per label), a scan over "I am that slot" for
// the component numbers, a stable radix sort of the slots by component for the CSR.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "device_common.hpp"
#include "kernels.hpp"
#include "lf_device.hpp"

namespace gbwt_hip {

namespace {


// slot of a GBWT node inside the alphabet, or COMPONENT_NONE outside it
__device__ __forceinline__ uint32_t slot_of(const DeviceIndex &ix, const ComponentGeometry &g, uint64_t node) {
    if (node < ix.first_node || node - ix.alphabet_offset >= ix.n_records) return COMPONENT_NONE;
    return static_cast<uint32_t>((node >> 1) - g.min_node);
}

// GBZ::has_node for slot s: the rule of k_mask_label_lengths (record_is_real) on the forward record of the slot
__device__ __forceinline__ bool slot_exists(const DeviceIndex &ix, const ComponentGeometry &g, uint64_t s) {
    const uint64_t forward = 2 * (g.min_node + s);
    return forward >= ix.first_node && record_is_real(ix, forward - ix.alphabet_offset);
}

__global__ void __launch_bounds__(256) k_component_init(uint32_t *parent, uint64_t slots) {
    const uint64_t s = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (s < slots) parent[s] = static_cast<uint32_t>(s);
}

__global__ void __launch_bounds__(256) k_hook(DeviceIndex ix, ComponentGeometry g, uint32_t *parent, uint32_t *changed) {
    const uint64_t rec = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x + 1;      // (record 0 is the endmarker's)
    if (rec >= ix.n_records) return;
    uint64_t start, limit;
    record_bounds(ix, rec, start, limit);
    if (start >= limit || limit > ix.data_len) return;
    const uint32_t u = static_cast<uint32_t>(((ix.alphabet_offset + rec) >> 1) - g.min_node);
    ByteCursor c(ix.data, start, limit);
    uint64_t sigma;
    if (!c.varint(sigma)) return;
    const uint32_t pu = parent[u];
    uint64_t node = 0;
    for (uint64_t e = 0; e < sigma; e++) {
        uint64_t delta, offset;
        if (!c.varint(delta) || !c.varint(offset)) break;     // (a header that ends inside the record's bytes: nothing is read past them)
        node += delta;
        if (node == 0) continue;                               // the ENDMARKER
        const uint32_t v = slot_of(ix, g, node);
        if (v == COMPONENT_NONE || v == u) continue;
        uint64_t a, b;
        record_bounds(ix, node - ix.alphabet_offset, a, b);
        if (a >= b) continue;                                  // a successor without a record
        const uint32_t pv = parent[v];
        if (pv == pu) continue;
        const uint32_t hi = pv > pu ? pv : pu, lo = pv > pu ? pu : pv;
        if (atomicMin(&parent[hi], lo) > lo) *changed = 1u;
    }
}

__global__ void __launch_bounds__(256) k_jump(uint32_t *parent, uint64_t slots, uint32_t *changed) {
    const uint64_t s = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (s >= slots) return;
    const uint32_t p = parent[s];
    const uint32_t q = parent[p];
    if (q != p) { parent[s] = q; *changed = 1u; }
}

// first[label] = the smallest slot of the component that exists (first[] preset to COMPONENT_NONE)
__global__ void __launch_bounds__(256) k_first_existing(DeviceIndex ix, ComponentGeometry g, const uint32_t *label, uint32_t *first) {
    const uint64_t s = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (s >= g.slots || !slot_exists(ix, g, s)) return;
    atomicMin(&first[label[s]], static_cast<uint32_t>(s));
}

__global__ void __launch_bounds__(256) k_is_first(const uint32_t *label, const uint32_t *first, uint64_t slots, uint32_t *flag) {
    const uint64_t s = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (s < slots) flag[s] = first[label[s]] == s ? 1u : 0u;
}

// component[s] = the rank of the component's first existing slot (COMPONENT_NONE for a slot that does not exist); key[s] = the same with
// `components` in place of COMPONENT_NONE (sorted behind every component), value[s] = s.  In place: `component` may be `label`.
__global__ void __launch_bounds__(256) k_component_numbers(DeviceIndex ix, ComponentGeometry g, const uint32_t *label, const uint32_t *first, const uint32_t *rank,
                                                            const uint32_t *flag, uint32_t *component, uint32_t *key, uint32_t *value) {
    const uint64_t s = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (s >= g.slots) return;
    const uint32_t components = rank[g.slots - 1] + flag[g.slots - 1];
    uint32_t c = COMPONENT_NONE;
    if (slot_exists(ix, g, s)) c = rank[first[label[s]]];
    component[s] = c;
    key[s] = c == COMPONENT_NONE ? components : c;
    value[s] = static_cast<uint32_t>(s);
}

__global__ void __launch_bounds__(256) k_component_counts(const uint32_t *component, uint64_t slots, unsigned long long *counts) {
    const uint64_t s = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (s < slots && component[s] != COMPONENT_NONE) atomicAdd(&counts[component[s]], 1ull);
}

// the sorted slots as node ids; the slots that do not exist lie behind them (key = components) and write nothing
__global__ void __launch_bounds__(256) k_slots_to_nodes(const uint32_t *sorted_keys, const uint32_t *sorted_slots, uint64_t slots, uint32_t components, uint32_t min_node,
                                                         uint32_t *out) {
    const uint64_t k = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (k < slots && sorted_keys[k] < components) out[k] = sorted_slots[k] + min_node;
}

// the component of path p = the component of the first node of its forward sequence (endmarker[sequence].x; 0: the path is empty)
__global__ void __launch_bounds__(256) k_path_components(DeviceIndex ix, ComponentGeometry g, const uint32_t *component, uint64_t paths, uint32_t stride, uint32_t *out) {
    const uint64_t p = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (p >= paths) return;
    const uint64_t seq = p * stride;
    uint32_t c = COMPONENT_NONE;
    if (seq < ix.n_endmarker) {
        const uint32_t s = slot_of(ix, g, ix.endmarker[seq].x);
        if (s != COMPONENT_NONE) c = component[s];
    }
    out[p] = c;
}

}  // namespace

void launch_component_init(uint32_t *d_parent, uint64_t slots, hipStream_t s) {
    if (slots) hipLaunchKernelGGL(k_component_init, dim3(blocks_for(slots)), dim3(256), 0, s, d_parent, slots);
}

void launch_component_hook(const DeviceIndex &ix, const ComponentGeometry &g, uint32_t *d_parent, uint32_t *d_changed, hipStream_t s) {
    if (ix.n_records > 1) hipLaunchKernelGGL(k_hook, dim3(blocks_for(ix.n_records - 1)), dim3(256), 0, s, ix, g, d_parent, d_changed);
}

void launch_component_jump(uint32_t *d_parent, uint64_t slots, uint32_t *d_changed, hipStream_t s) {
    if (slots) hipLaunchKernelGGL(k_jump, dim3(blocks_for(slots)), dim3(256), 0, s, d_parent, slots, d_changed);
}

size_t component_shape_temp_bytes(uint64_t slots) {
    size_t scan = 0, sort = 0;
    const int n = static_cast<int>(slots);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan, static_cast<const uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr), n);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sort, static_cast<const uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr), static_cast<const uint32_t *>(nullptr),
                                             static_cast<uint32_t *>(nullptr), n, 0, 32);
    return std::max(scan, sort);
}

void launch_component_numbers(const DeviceIndex &ix, const ComponentGeometry &g, const ComponentShape &w, hipStream_t s) {
    if (g.slots == 0) return;
    const unsigned blocks = blocks_for(g.slots);
    size_t temp = w.temp_bytes;
    (void)hipMemsetAsync(w.first, 0xFF, g.slots * sizeof(uint32_t), s);
    hipLaunchKernelGGL(k_first_existing, dim3(blocks), dim3(256), 0, s, ix, g, w.label, w.first);
    hipLaunchKernelGGL(k_is_first, dim3(blocks), dim3(256), 0, s, w.label, w.first, g.slots, w.flag);
    (void)hipcub::DeviceScan::ExclusiveSum(w.temp, temp, w.flag, w.rank, static_cast<int>(g.slots), s);
    hipLaunchKernelGGL(k_component_numbers, dim3(blocks), dim3(256), 0, s, ix, g, w.label, w.first, w.rank, w.flag, w.label, w.key, w.value);
}

void launch_component_counts(const ComponentGeometry &g, const uint32_t *d_component, uint64_t components, uint64_t *d_counts, hipStream_t s) {
    if (g.slots == 0 || components == 0) return;
    (void)hipMemsetAsync(d_counts, 0, components * sizeof(uint64_t), s);
    hipLaunchKernelGGL(k_component_counts, dim3(blocks_for(g.slots)), dim3(256), 0, s, d_component, g.slots, reinterpret_cast<unsigned long long *>(d_counts));
}

void launch_component_csr(const ComponentGeometry &g, const ComponentShape &w, uint64_t components, uint32_t *d_nodes, hipStream_t s) {
    if (g.slots == 0) return;
    size_t temp = w.temp_bytes;
    int bits = 1;
    while (bits < 32 && (components >> bits) != 0) bits++;                 // keys are 0 .. components
    (void)hipcub::DeviceRadixSort::SortPairs(w.temp, temp, w.key, w.first, w.value, w.rank, static_cast<int>(g.slots), 0, bits, s);   // (first / rank are free by now)
    hipLaunchKernelGGL(k_slots_to_nodes, dim3(blocks_for(g.slots)), dim3(256), 0, s, w.first, w.rank, g.slots, static_cast<uint32_t>(components), static_cast<uint32_t>(g.min_node), d_nodes);
}

void launch_path_components(const DeviceIndex &ix, const ComponentGeometry &g, const uint32_t *d_component, uint64_t paths, uint32_t stride, uint32_t *d_out, hipStream_t s) {
    if (paths) hipLaunchKernelGGL(k_path_components, dim3(blocks_for(paths)), dim3(256), 0, s, ix, g, d_component, paths, stride, d_out);
}

}  // namespace gbwt_hip
