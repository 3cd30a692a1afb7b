// handle.hpp -- gbwt_hip_index, the handle of the C ABI: the host image, the arrays in HBM that an open makes, and the parts that the first
// request for them makes (labels, components, the locate index).
#pragma once

#include <chrono>
#include <memory>
#include <vector>

#include "capi_status.hpp"
#include "device_buffer.hpp"
#include "device_index.hpp"
#include "host_index.hpp"
#include "kernels.hpp"
#include "knobs.hpp"
#include "lazy_build.hpp"

namespace gbwt_hip {

// The parts of a handle in HBM that no open makes: each is built by the first request that needs it, once per handle whichever thread asks
// first, and counted by gbwt_hip_memory_usage once built.made().  release(): what a build that failed half-way gives back.

// NODE LABELS (sequences.hip: ensure_labels), made by the first request for bases: the bytes of every potential node's label (+ 64 zero
// bytes, so that the aligned dword loads of the bases kernel may read past the last one) and u64 offsets[nodes + 1].
struct LazyLabels {
    LazyBuild built;
    DeviceBuffer bytes, off;
    uint64_t device_bytes() const { return bytes_of({&bytes, &off}); }
    void release() { bytes.release(); off.release(); max_len = 0; }
    uint64_t max_len = 0;
};

// WEAKLY CONNECTED COMPONENTS (capi_graph.hip: ensure_components), made by the first call that asks for them: the component of every node
// slot, the CSR of the components (u64 offsets, u32 node ids) and the component of every path; the path components on the host as well
// (what select_paths reads).
struct LazyComponents {
    LazyBuild built;
    DeviceBuffer of, offsets, nodes, paths;
    uint64_t device_bytes() const { return bytes_of({&of, &offsets, &nodes, &paths}); }
    void release() { of.release(); offsets.release(); nodes.release(); paths.release(); host_paths.clear(); count = node_count = 0; }
    ComponentGeometry geometry{0, 0};
    uint64_t count = 0, node_count = 0;
    std::vector<uint32_t> host_paths;
    gbwt_hip_components_times times{};
};

// THE LOCATE INDEX (locate.hip, capi_locate.hip: ensure_locate), made by the first locate call: the table base of every record (u64,
// LOCATE_NONE where the record is not sampled), the sequence id of every position of a sampled record (u32) and the sorted end entries of
// the sequences.  A build that fails keeps nothing.
struct LazyLocate {
    LazyBuild built;
    DeviceBuffer base, table, end_keys, end_ids;
    uint64_t device_bytes() const { return bytes_of({&base, &table, &end_keys, &end_ids}); }
    void release() { base.release(); table.release(); end_keys.release(); end_ids.release(); index = LocateIndex{nullptr, nullptr, nullptr, nullptr, 0, 0}; }
    LocateIndex index{nullptr, nullptr, nullptr, nullptr, 0, 0};
    uint64_t sampled_records = 0;
    float build_ms = 0;
    uint32_t build_launches = 0;
};

}  // namespace gbwt_hip

struct gbwt_hip_index {
    gbwt_hip::HostIndex host;
    int device = 0;
    OpenKnobs knobs;                      // the open's settings (gbwt_hip_open_*_flags)
    bool lean_extract = false;           // opened without SEARCH and no record needs the generic decoder: desc_raw was given back after the open (capi_open.hip: open_common)
    uint64_t slow_records = ~uint64_t(0); // non-empty records whose walk descriptor says "generic decoder" (k_link_desc2's count; ~0 = not counted)
    uint32_t caps = GBWT_HIP_OPEN_ALL;   // what the handle was opened for (gbwt_hip_open_*_flags): which arrays exist, which entry points answer
    uint64_t table_positions = 0;     // BWT positions in records with LF tables (outdegree > 2)
    gbwt_hip::DeviceBuffer data, starts, endmarker, desc, desc_raw, block_base, blocks, desc2, cblocks, gblocks, tables, wtables, wtables_deep, seq_len, samples, sample_base;
    gbwt_hip::DeviceBuffer label_len;   // GBZ only: label length per potential node (0 for nodes that do not exist)
    // GBZ with a node-to-segment translation (src/graph.rs:186-218), flattened for the line formatter:
    gbwt_hip::DeviceBuffer seg_of;        // u32 per node id < mapping_len: segment holding the node (~0 before the first segment)
    gbwt_hip::DeviceBuffer seg_start;     // u32 per segment + 1: first node id of the segment, last = mapping_len
    gbwt_hip::DeviceBuffer seg_name_off;  // u64 per segment + 1: offsets into seg_names
    gbwt_hip::DeviceBuffer seg_names;     // segment names, concatenated
    gbwt_hip::DeviceBuffer seg_seq_len;   // u64 per segment: length of the segment's sequence
    gbwt_hip::DeviceBuffer node_real;     // u8 per node id < mapping_len: GBZ::has_node
    // GFA line headers, one table per line mode (0 = P-line named by the contig, 1 = W-line, 2 = P-line with the PanSN name): for every path of
    // the metadata the bytes of its line up to the node tokens -- for a W-line up to and including "<fragment>\t"; the end coordinate
    // (fragment + summed label lengths, path_to_w_line, src/bin/gbunzip.rs:532-540) is only known once the path has been walked and is
    // appended by the device.  Built once at open (open_lines.hip: upload_label_lengths), so that a request formats its lines without the host.
    gbwt_hip::DeviceBuffer line_prefix[3], line_prefix_off[3], line_fragment;
    std::vector<char> host_line_prefix[3];
    std::vector<uint64_t> host_line_prefix_off[3];
    // LINE CACHE (open_lines.hip fills it, capi_lines.hip reads it): what the GFA line of a path is made of -- the text bytes of its node tokens, chunk by chunk, and its summed label
    // lengths (the W-line's end coordinate) -- is a property of the index, not of the request.  Round 5 let the first request that formats a
    // path leave them here; since round 6 ONE walk at open fills them for every path (fill_line_cache_at_open; kernels.hpp: LineCacheFill), so
    // that no request sizes a line: the node ids cross HBM twice (written by the walk, read by the formatter), never three times.
    // 8 bytes per 4 096 path positions + 16 per path.  Absent (-1) without sequence samples, for graphs with a node-to-segment translation
    // and with GBWT_HIP_LINE_CACHE=0: requests then size their lines themselves (k_chunk_stats).
    gbwt_hip::DeviceBuffer lc_chunk_first, lc_text, lc_path;    // u64[paths + 1]: first chunk of every path; u64 per chunk: W-token bytes of the path in front of it; u64[2] per path: {W-token bytes, summed label lengths}
    int lc_state = 0;                                             // 1 = filled at open, -1 = not for this index (written before the handle is handed out)
    // every buffer above that an open makes; cblocks at open or by the first request that needs them (below); the three parts below once made
    uint64_t device_bytes() const {
        return gbwt_hip::bytes_of({&data, &starts, &endmarker, &desc, &desc_raw, &block_base, &blocks, &desc2, &gblocks, &tables, &wtables, &wtables_deep, &seq_len, &samples,
                                   &sample_base, &label_len, &seg_of, &seg_start, &seg_name_off, &seg_names, &seg_seq_len, &node_real, &line_prefix[0], &line_prefix[1],
                                   &line_prefix[2], &line_prefix_off[0], &line_prefix_off[1], &line_prefix_off[2], &line_fragment, &lc_chunk_first, &lc_text, &lc_path}) +
               (dev.cblocks != nullptr || cblocks_built.made() ? cblocks.bytes : 0) + (labels.built.made() ? labels.device_bytes() : 0) +
               (components.built.made() ? components.device_bytes() : 0) + (locate.built.made() ? locate.device_bytes() : 0);
    }
    std::vector<uint32_t> host_seq_len;   // host copy of seq_len (empty when the lengths are not known): sizes byte-bounded batches of a whole-file write
    // made by the first request that needs them, never by an open (above)
    mutable gbwt_hip::LazyLabels labels;
    mutable gbwt_hip::LazyComponents components;
    mutable gbwt_hip::LazyLocate locate;
    gbwt_hip::DeviceIndex dev{};
    // The full-width two-step blocks (cblocks, as large as gblocks: 1.7 GB on the headline index) are only read by the loops for records
    // whose counts do not fit the packed half-blocks, by the pool-output kernel and by the serial walks at open: built at open when one of
    // those is certain to run, else on the first request that needs them (ensure_cblocks; once, whichever thread comes first).
    mutable gbwt_hip::LazyBuild cblocks_built;
    bool packed_blocks = false;       // gblocks holds the packed half-blocks (set by the open's walk layout, capi_open.hip: layout_walks; false: a handle
                                      // not opened for extraction, an index too large for 32-bit half-block indices, or GBWT_HIP_GATHER_LIMIT=0)
    uint32_t max_samples = 0;         // the largest number of samples of a sequence
    uint32_t sample_coarse = 1;       // the samples are this many times finer than a batch of the whole index wants: extractions stride over them (capi_extract.hip)
    std::vector<uint32_t> sample_counts;   // samples of every sequence (host copy: an extraction looks whether its rows all have the same number)
    uint32_t uniform_samples = 0;     // every sequence has this many samples (0: they differ): the walkers of an extraction are then w = segment * n + row
    bool starts_uploaded = false;         // ... and the record starts
    bool record_bytes_uploaded = false;   // gbwt_hip_open_file has copied the record bytes to `data` while the loader was still decoding
    gbwt_hip_open_times times{};      // where the time of the open went (gbwt_hip_get_open_times)
    gbwt_hip_build_info build_info{}; // the construction behind the handle (capi_build.hip); zeros for a handle that was opened from a file or from records
    gbwt_hip_gfa_info gfa_info{};     // the parse behind a handle made from GFA (capi_gfa_build.hip); zeros for every other handle
    gbwt_hip_gfa_translation_info gfa_translation_info{};   // its translation, if it made one
    gbwt_hip_merge_info merge_info{};   // the merge behind the handle (capi_merge.hip); zeros for every other handle
    gbwt_hip_remove_info remove_info{}; // the removal behind the handle (capi_remove.hip); zeros for every other handle
    uint32_t uniform_len = 0;         // every sequence has this many nodes (0: lengths differ, or unknown): an extraction then knows its offsets without asking the device
    bool orientation_pairs = false;   // verified at open: sequence 2k + 1 is sequence 2k reversed (rows can be filled from both ends)
    gbwt_hip_stats stats{};
};

namespace gbwt_hip {
// A handle with its settings and nothing else: the device, what it is opened for (caps decide which arrays the open makes) and the
// GBWT_HIP_* settings of the open, read here and nowhere else
inline std::unique_ptr<gbwt_hip_index> new_handle(int device, uint32_t flags) {
    std::unique_ptr<gbwt_hip_index> ix(new gbwt_hip_index);
    ix->device = device;
    ix->caps = normalised_caps(flags);
    ix->knobs = OpenKnobs::from_env();
    return ix;
}

// gbwt_hip_last_*_info, gbwt_hip_get_stats, gbwt_hip_get_open_times: a struct the open or a maker left on the handle
// (static, like fill_build_counters and extract_rows: a helper over the ABI's types adds no symbol to what the library exports)
template <class Info>
static gbwt_hip_status last_info(const gbwt_hip_index *ix, Info *out, Info gbwt_hip_index::*member) {
    if (!ix || !out) return fail(GBWT_HIP_BAD_ARGUMENT, "null argument");
    *out = ix->*member;
    return GBWT_HIP_OK;
}

// capi_open.hip: the open behind every handle -- device passes, GFA tables, line cache -- for a host image that is already filled (takes
// ownership; t_open: when the caller started, for the handle's open times).  Settings come with the handle (new_handle).
gbwt_hip_status open_host_index(std::unique_ptr<gbwt_hip_index> ix, gbwt_hip_index **out, std::chrono::steady_clock::time_point t_open);

// The full-width two-step blocks of a handle, built on first need, and a copy of its DeviceIndex with them put in (capi_open.hip)
const uint4 *ensure_cblocks(const gbwt_hip_index *index);
DeviceIndex with_cblocks(const gbwt_hip_index *ix);


}  // namespace gbwt_hip
