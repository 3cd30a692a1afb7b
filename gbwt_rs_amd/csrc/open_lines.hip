// open_lines.hip -- what an open with GBWT_HIP_OPEN_GFA leaves in the handle for the GFA lines (capi_open.hip: open_common calls these):
// the label length of every node, the header of every path's line in the three line modes, the node-to-segment translation flattened,
// and the line cache.  Host code over gbwt_hip_index; the kernels it launches are load_kernels.hip's and open_walks.hip's.
#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>

#include "capi_internal.hpp"
#include "gfa_host.hpp"
#include "lines_plan.hpp"

namespace gbwt_hip {

// The header of every path's line in the three line modes, up to the node tokens (path_to_p_line / path_to_pan_sn / path_to_w_line,
// src/bin/gbunzip.rs:480-524; Metadata::pan_sn_path, src/gbwt.rs:709-713; sample_name / contig_name fall back to the number,
// src/gbwt.rs:744-761, 792-809).  A W-line's end coordinate follows its fragment field and is appended on the device.
static void upload_line_headers(gbwt_hip_index &ix) {
    const HostIndex &h = ix.host;
    if (!h.has_metadata || h.path_names.empty()) return;
    const bool sample_names = (h.metadata_flags & 2) != 0, contig_names = (h.metadata_flags & 4) != 0;
    const uint64_t n = h.path_names.size();
    std::vector<uint32_t> fragment(n);
    for (uint64_t p = 0; p < n; p++) fragment[p] = h.path_names[p].fragment;
    auto build = [&](int mode) {
        std::vector<char> &out = ix.host_line_prefix[mode];
        std::vector<uint64_t> &off = ix.host_line_prefix_off[mode];
        out.clear(); out.reserve(32 * n);
        off.assign(n + 1, 0);
        auto text = [&](const char *t) { while (*t) out.push_back(*t++); };
        auto number = [&](uint64_t v) {
            char digits[24];
            int len = 0;
            do { digits[len++] = static_cast<char>('0' + v % 10); v /= 10; } while (v != 0);
            while (len > 0) out.push_back(digits[--len]);
        };
        auto name = [&](const Strings &names, bool has_names, uint64_t id) {
            if (has_names && id < names.size()) out.insert(out.end(), names.bytes.begin() + names.offsets[id], names.bytes.begin() + names.offsets[id + 1]);
            else number(id);
        };
        for (uint64_t p = 0; p < n; p++) {
            const PathName &pn = h.path_names[p];
            if (mode == 0) { text("P\t"); name(h.contig_names, contig_names, pn.contig); out.push_back('\t'); }
            else if (mode == 2) {
                text("P\t"); name(h.sample_names, sample_names, pn.sample); out.push_back('#'); number(pn.phase); out.push_back('#');
                name(h.contig_names, contig_names, pn.contig); out.push_back('\t');
            } else {
                text("W\t"); name(h.sample_names, sample_names, pn.sample); out.push_back('\t'); number(pn.phase); out.push_back('\t');
                name(h.contig_names, contig_names, pn.contig); out.push_back('\t'); number(pn.fragment); out.push_back('\t');
            }
            off[p + 1] = out.size();
        }
    };
    std::thread others[2] = {std::thread(build, 0), std::thread(build, 2)};    // (tens of thousands of walks in a config-4-shaped GBZ)
    build(1);
    for (auto &t : others) t.join();
    for (int mode = 0; mode < 3; mode++) {
        ix.line_prefix[mode].reserve(std::max<size_t>(ix.host_line_prefix[mode].size(), 16));
        ix.line_prefix_off[mode].reserve((n + 1) * sizeof(uint64_t));
        if (!ix.host_line_prefix[mode].empty())
            HIP_CHECK(hipMemcpy(ix.line_prefix[mode].ptr, ix.host_line_prefix[mode].data(), ix.host_line_prefix[mode].size(), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(ix.line_prefix_off[mode].ptr, ix.host_line_prefix_off[mode].data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    ix.line_fragment.reserve(n * sizeof(uint32_t));
    HIP_CHECK(hipMemcpy(ix.line_fragment.ptr, fragment.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
}

// Uploads the label length of every potential node; mask_label_lengths below then zeroes those of the nodes that do not exist (GBZ::has_node,
// src/gbz.rs:286-289) ON THE DEVICE, from the record bytes and starts there -- the host's image of them is not made by an open
// (HostIndex::ensure_records), and the device passes that put them there may still be running on another thread when this one is.
void upload_label_lengths(gbwt_hip_index &ix) {
    const HostIndex &h = ix.host;
    if (!h.is_gbz) return;
    std::vector<uint32_t, DefaultInitAllocator<uint32_t>> len(h.sequences_labels.size() + 1);
    len.back() = 0;
    {   // (sixteen million nodes in a config-4-shaped GBZ: a few threads)
        const uint64_t n = h.sequences_labels.size();
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const unsigned pieces = n >= (uint64_t(1) << 23) ? std::max(std::min(8u, hw), std::min(static_cast<unsigned>(std::min<uint64_t>(n >> 21, 32)), hw)) : 1u;   // (109 M nodes: 32 threads)
        auto piece = [&](unsigned p) {
            for (uint64_t s = n * p / pieces, end = n * (p + 1) / pieces; s < end; s++) len[s] = static_cast<uint32_t>(h.sequences_labels.len(s));
        };
        std::vector<std::thread> pool;
        for (unsigned p = 1; p < pieces; p++) pool.emplace_back(piece, p);
        piece(0);
        for (auto &t : pool) t.join();
    }
    ix.label_len.reserve(len.size() * sizeof(uint32_t));
    HIP_CHECK(hipMemcpy(ix.label_len.ptr, len.data(), len.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    upload_line_headers(ix);
    if (!h.has_translation || h.segment_starts.empty()) return;
    // node-to-segment translation, flattened (Graph::node_to_segment is a predecessor query on a sparse vector in the
    // reference, src/graph.rs:186-198; here every node id gets its segment)
    if (h.mapping_len >= 0xFFFFFFFFull) throw InvalidData("Graph: node ids of the translation do not fit 32 bits");
    const uint64_t n_seg = h.segment_starts.size();
    std::vector<uint32_t> seg_of(h.mapping_len, 0xFFFFFFFFu), seg_start(n_seg + 1);
    std::vector<uint64_t> seq_len(n_seg);
    std::vector<uint8_t> node_real(h.mapping_len, 0);
    for (uint64_t s = 0; s < n_seg; s++) {
        const HostSegment seg = host_segment(h, s);
        if (seg.start == 0 || seg.end > h.mapping_len || seg.end < seg.start) throw InvalidData("Graph: malformed node-to-segment mapping");
        seg_start[s] = static_cast<uint32_t>(seg.start);
        for (uint64_t v = seg.start; v < seg.end; v++) seg_of[v] = static_cast<uint32_t>(s);
        seq_len[s] = host_segment_seq_len(h, seg);
    }
    seg_start[n_seg] = static_cast<uint32_t>(h.mapping_len);
    for (uint64_t v = 0; v < h.mapping_len; v++) node_real[v] = node_exists(h, v) ? 1 : 0;
    auto put = [](DeviceBuffer &b, const void *src, size_t bytes) {
        b.reserve(std::max<size_t>(bytes, 16));
        if (bytes) HIP_CHECK(hipMemcpy(b.ptr, src, bytes, hipMemcpyHostToDevice));
    };
    put(ix.seg_of, seg_of.data(), seg_of.size() * sizeof(uint32_t));
    put(ix.seg_start, seg_start.data(), seg_start.size() * sizeof(uint32_t));
    put(ix.seg_name_off, h.segment_names.offsets.data(), h.segment_names.offsets.size() * sizeof(uint64_t));
    put(ix.seg_names, h.segment_names.bytes.data(), h.segment_names.bytes.size());
    put(ix.seg_seq_len, seq_len.data(), seq_len.size() * sizeof(uint64_t));
    put(ix.node_real, node_real.data(), node_real.size());
}

void mask_label_lengths(gbwt_hip_index &ix) {
    if (!ix.host.is_gbz || ix.label_len.ptr == nullptr) return;
    launch_mask_label_lengths(ix.dev, ix.label_len.as<uint32_t>(), ix.host.sequences_labels.size(), nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
}

// The line cache of a handle, filled by ONE walk at open (kernels.hpp: LineCacheFill; open_walks.hip: k_segment_text): usable when the index
// has sequence samples (the walkers start from them, as those of an extraction do) and the graph has no node-to-segment translation
// (tokens are then segment names, sized by other rules).  Called by open_common once the device passes and the GFA tables are done, while
// the raw descriptors are still there (slow records take the generic decoder).
void fill_line_cache_at_open(gbwt_hip_index &ix) {
    const HostIndex &h = ix.host;
    ix.lc_state = -1;
    const uint64_t paths = h.path_names.size();
    const bool translated = h.has_translation && !h.segment_starts.empty();
    if (!(ix.caps & GBWT_HIP_OPEN_GFA) || !h.is_gbz || !h.has_metadata || translated || paths == 0 || !ix.knobs.line_cache) return;
    if (ix.host_seq_len.size() < 2 * paths || ix.sample_counts.size() < 2 * paths || 2 * paths > h.sequences) return;
    const DeviceIndex &d = ix.dev;
    if (d.samples == nullptr || d.sample_base == nullptr || d.seq_len == nullptr || d.desc2 == nullptr || (!ix.packed_blocks && d.cblocks == nullptr)) return;
    if (ix.label_len.ptr == nullptr) return;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> first(paths + 1, 0);
    uint32_t max_samples = 0;
    for (uint64_t p = 0; p < paths; p++) {
        const uint64_t len = ix.host_seq_len[2 * p];                   // the forward sequence of path p (support::encode_path)
        first[p + 1] = first[p] + (len == 0 ? 1 : (len + LINE_CHUNK - 1) / LINE_CHUNK);
        max_samples = std::max(max_samples, ix.sample_counts[2 * p]);
    }
    if (static_cast<uint64_t>(max_samples) * paths > (uint64_t(1) << 36)) return;      // (walkers = most samples of a path x paths: beyond any launch; such a handle sizes per request)
    HIP_CHECK(hipSetDevice(ix.device));
    ix.lc_chunk_first.reserve((paths + 1) * sizeof(uint64_t));
    ix.lc_text.reserve(std::max<uint64_t>(first[paths], 1) * sizeof(uint64_t));
    ix.lc_path.reserve(2 * paths * sizeof(uint64_t));
    HIP_CHECK(hipMemcpy(ix.lc_chunk_first.ptr, first.data(), (paths + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    DeviceBuffer chunk_seg, seg_text, flags;
    chunk_seg.reserve(std::max<uint64_t>(first[paths], 1) * sizeof(uint32_t));
    seg_text.reserve(std::max<uint64_t>(ix.times.samples, 1) * 2 * sizeof(uint64_t));
    flags.reserve(sizeof(uint32_t));
    HIP_CHECK(hipMemsetAsync(flags.ptr, 0, sizeof(uint32_t), nullptr));
    HIP_CHECK(hipMemsetAsync(ix.lc_text.ptr, 0, std::max<uint64_t>(first[paths], 1) * sizeof(uint64_t), nullptr));
    HIP_CHECK(hipMemsetAsync(chunk_seg.ptr, 0, std::max<uint64_t>(first[paths], 1) * sizeof(uint32_t), nullptr));
    LineCacheFill f{};
    f.label_len = ix.label_len.as<uint32_t>(); f.n_labels = h.sequences_labels.size(); f.paths = paths; f.max_samples = max_samples;
    f.chunk_first = ix.lc_chunk_first.as<uint64_t>(); f.chunks = first[paths]; f.chunk_text = ix.lc_text.as<uint64_t>(); f.path_totals = ix.lc_path.as<uint64_t>();
    f.chunk_seg = chunk_seg.as<uint32_t>(); f.seg_text = seg_text.as<uint64_t>(); f.flags = flags.as<uint32_t>();
    launch_fill_line_cache(d, f, ix.packed_blocks, nullptr);
    uint32_t bad = 0;
    HIP_CHECK(hipMemcpy(&bad, flags.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipGetLastError());
    if (bad != 0) {                                                    // samples that promise more nodes than the walk delivers: requests size their lines themselves
        ix.lc_chunk_first.release(); ix.lc_text.release(); ix.lc_path.release();
        return;
    }
    ix.lc_state = 1;
    ix.times.line_sizes_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace gbwt_hip
