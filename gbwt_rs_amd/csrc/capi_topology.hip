// capi_topology.hip -- the graph over the C ABI (include/gbwt_hip.h, "the graph"): node ids, edge rows, segments, link rows and the H-, S-
// and L-lines of a GFA file, computed by the kernels of topology.hip from the record bytes, the translation tables and the labels in HBM.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "capi_internal.hpp"
#include "gfa_host.hpp"
#include "scan.hpp"
#include "topology.hpp"

using namespace gbwt_hip;

namespace {

GraphTables graph_tables(const gbwt_hip_index *ix, bool with_labels) {
    const HostIndex &h = ix->host;
    GraphTables t{};
    if (h.is_gbz && h.has_translation && !h.segment_starts.empty() && ix->seg_start.ptr) {
        t.seg_of = ix->seg_of.as<uint32_t>(); t.seg_start = ix->seg_start.as<uint32_t>(); t.name_off = ix->seg_name_off.as<uint64_t>();
        t.names = ix->seg_names.as<uint8_t>(); t.seq_len = ix->seg_seq_len.as<uint64_t>(); t.node_real = ix->node_real.as<uint8_t>();
        t.mapping_len = h.mapping_len; t.segments = h.segment_starts.size();
    }
    if (with_labels) {
        const Labels l = labels_of(ix);
        t.label_bytes = l.bytes; t.label_off = l.off; t.labels = l.n; t.first_node = l.first_node;
    }
    return t;
}

void scan(gbwt_hip_workspace *ws, const uint64_t *d_lengths, uint64_t *d_offsets, uint64_t n, hipStream_t s) {
    const size_t temp = scan_temp_bytes(n, ws->knobs.scan_piece);
    ws->scratch.scan_temp.reserve(temp);
    launch_scan(d_lengths, d_offsets, n, ws->scratch.scan_temp.ptr, temp, s, ws->knobs.scan_piece);
}

const char *const NEEDS_GFA = "segments, links and graph lines need a GBZ opened with GBWT_HIP_OPEN_GFA";

// The rows of a request, computed once into the workspace: edge rows (edges.off / edges.edges) or, links != 0, link rows (edges.loff / edges.links);
// edges.valid, edges.total.  The request is remembered: the fill call after a size query finds its rows here.
gbwt_hip_status rows_compute(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *ids, const uint8_t *orientations, uint64_t n, int predecessors, int links) {
    if (!ix || !ws || ws->index != ix) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    if (n && (!ids || !orientations)) return fail(GBWT_HIP_BAD_ARGUMENT, "null ids / orientations");
    if (n >= 0xFFFFFFFFull) return fail(GBWT_HIP_BAD_ARGUMENT, "too many rows in one request (32-bit row numbers)");
    if (links && (!ix->host.is_gbz || !(ix->caps & GBWT_HIP_OPEN_GFA))) return fail(GBWT_HIP_BAD_ARGUMENT, NEEDS_GFA);
    predecessors = predecessors ? 1 : 0;
    const size_t id_bytes = n * sizeof(uint64_t);
    if (ws->edges.memo.matches({{ids, id_bytes}, {orientations, n}}, {links, predecessors, static_cast<int64_t>(n)})) return GBWT_HIP_OK;
    ws->edges.memo.drop();
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        hipStream_t s = ws->stream;
        const uint64_t rows = std::max<uint64_t>(n, 1);
        ws->edges.ids.reserve(rows * sizeof(uint64_t));
        ws->edges.orient.reserve(rows);
        ws->edges.counts.reserve(rows * sizeof(uint64_t));
        ws->edges.off.reserve((rows + 1) * sizeof(uint64_t));
        ws->edges.valid.reserve(rows);
        ws->edges.big.reserve((rows + 1) * sizeof(uint32_t));
        ws->query.ev.ensure();
        const GraphTables tables = links ? graph_tables(ix, false) : GraphTables{};
        if (links) {
            ws->edges.seg.reserve(rows * (sizeof(uint64_t) + 1));
            uint8_t *d_seg_orient = ws->edges.seg.as<uint8_t>() + rows * sizeof(uint64_t);
            if (n) {
                HIP_CHECK(hipMemcpyAsync(ws->edges.seg.ptr, ids, id_bytes, hipMemcpyHostToDevice, s));
                HIP_CHECK(hipMemcpyAsync(d_seg_orient, orientations, n, hipMemcpyHostToDevice, s));
            }
            HIP_CHECK(hipEventRecord(ws->query.ev[0], s));
            launch_link_queries(tables, ws->edges.seg.as<uint64_t>(), d_seg_orient, n, predecessors != 0, ws->edges.ids.as<uint64_t>(), ws->edges.orient.as<uint8_t>(), s);
        } else {
            if (n) {
                HIP_CHECK(hipMemcpyAsync(ws->edges.ids.ptr, ids, id_bytes, hipMemcpyHostToDevice, s));
                HIP_CHECK(hipMemcpyAsync(ws->edges.orient.ptr, orientations, n, hipMemcpyHostToDevice, s));
            }
            HIP_CHECK(hipEventRecord(ws->query.ev[0], s));
        }
        launch_edge_count(ix->dev, ws->edges.ids.as<uint64_t>(), ws->edges.orient.as<uint8_t>(), n, predecessors != 0, ws->edges.counts.as<uint64_t>(), ws->edges.valid.as<uint8_t>(), s);
        scan(ws, ws->edges.counts.as<uint64_t>(), ws->edges.off.as<uint64_t>(), n, s);
        HIP_CHECK(hipGetLastError());
        uint64_t total = read_value(ws->edges.off.as<uint64_t>() + n, s);
        ws->edges.edges.reserve(std::max<uint64_t>(total, 1) * sizeof(uint64_t));
        if (links) ws->edges.rows.reserve(std::max<uint64_t>(total, 1) * sizeof(uint32_t));
        launch_edge_fill(ix->dev, ws->edges.ids.as<uint64_t>(), ws->edges.orient.as<uint8_t>(), n, predecessors != 0, ws->edges.off.as<uint64_t>(), ws->edges.edges.as<uint64_t>(),
                         links ? ws->edges.rows.as<uint32_t>() : nullptr, ws->edges.big.as<uint32_t>(), s);
        if (links) {
            ws->edges.cut.reserve(rows * sizeof(uint64_t));
            ws->edges.loff.reserve((rows + 1) * sizeof(uint64_t));
            launch_link_cut(tables, ws->edges.off.as<uint64_t>(), ws->edges.edges.as<uint64_t>(), ws->edges.rows.as<uint32_t>(), n, total, ws->edges.cut.as<uint64_t>(), s);
            scan(ws, ws->edges.cut.as<uint64_t>(), ws->edges.loff.as<uint64_t>(), n, s);
            HIP_CHECK(hipGetLastError());
            const uint64_t kept = read_value(ws->edges.loff.as<uint64_t>() + n, s);
            ws->edges.links.reserve(std::max<uint64_t>(kept, 1) * sizeof(uint64_t));
            launch_link_write(tables, ws->edges.off.as<uint64_t>(), ws->edges.edges.as<uint64_t>(), ws->edges.rows.as<uint32_t>(), total, ws->edges.cut.as<uint64_t>(),
                              ws->edges.loff.as<uint64_t>(), ws->edges.links.as<uint64_t>(), s);
            total = kept;
        }
        HIP_CHECK(hipEventRecord(ws->query.ev[1], s));
        ws->query.timed = true;
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        ws->edges.n = n; ws->edges.total = total;
        ws->edges.memo.store({{ids, id_bytes}, {orientations, n}}, {links, predecessors, static_cast<int64_t>(n)});
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
}

gbwt_hip_status rows_to_host(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *ids, const uint8_t *orientations, uint64_t n, int predecessors, int links,
                             uint64_t *out_offsets, uint64_t *out, uint64_t capacity, uint64_t *total, uint8_t *valid) {
    if (!total || !out_offsets || (n && !valid)) return fail(GBWT_HIP_BAD_ARGUMENT, "null buffer");
    *total = 0;
    out_offsets[0] = 0;
    const gbwt_hip_status st = rows_compute(ix, ws, ids, orientations, n, predecessors, links);
    if (st != GBWT_HIP_OK) return st;
    *total = ws->edges.total;
    if (n == 0) return GBWT_HIP_OK;
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        hipStream_t s = ws->stream;
        HIP_CHECK(hipMemcpyAsync(out_offsets, (links ? ws->edges.loff : ws->edges.off).ptr, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(valid, ws->edges.valid.ptr, n, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (!out) return GBWT_HIP_OK;
        if (capacity < *total) return fail(GBWT_HIP_CAPACITY, links ? "output capacity too small for the links" : "output capacity too small for the edges");
        if (*total) copy_to_host(ws, out, (links ? ws->edges.links : ws->edges.edges).ptr, *total * sizeof(uint64_t));
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
}

gbwt_hip_status rows_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *ids, const uint8_t *orientations, uint64_t n, int predecessors, int links,
                            gbwt_hip_edge_rows *out) {
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_edge_rows{nullptr, nullptr, nullptr, 0, 0};
    const gbwt_hip_status st = rows_compute(ix, ws, ids, orientations, n, predecessors, links);
    if (st != GBWT_HIP_OK) return st;
    out->d_offsets = (links ? ws->edges.loff : ws->edges.off).as<uint64_t>();
    out->d_edges = (links ? ws->edges.links : ws->edges.edges).as<uint64_t>();
    out->d_valid = ws->edges.valid.as<uint8_t>();
    out->total = ws->edges.total;
    out->n = n;
    return GBWT_HIP_OK;
}

// The sizes of the graph lines of a workspace's index, once: items and offsets of the S-lines, edge rows and offsets of the L-lines.
void graph_lines_size(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const GraphTables &t, const ComponentGeometry &g, hipStream_t s) {
    const HostIndex &h = ix->host;
    const bool translated = t.segments != 0;
    const uint64_t domain = translated ? t.segments : g.slots, queries = 2 * domain;
    if (queries >= 0xFFFFFFFFull) throw Unsupported("too many nodes for the graph lines (32-bit row numbers)");
    if (const std::string *rs = h.tag("reference_samples")) ws->graph_text.header = "H\tVN:Z:1.1\tRS:Z:" + *rs + "\n";      // write_gfa_header, src/bin/gbunzip.rs:193-203
    else ws->graph_text.header = "H\tVN:Z:1.1\n";
    DeviceBuffer flags, rank, sizes, ids, orient, counts, off, valid, big, cut, lines;
    // 1. the items of the S-lines: the nodes that exist, or the segments whose first node does (GBZ::segment_iter)
    flags.reserve(std::max<uint64_t>(domain, 1) * sizeof(uint64_t));
    rank.reserve((domain + 1) * sizeof(uint64_t));
    if (translated) launch_segment_flags(t, flags.as<uint64_t>(), s);
    else launch_node_flags(ix->dev, g, flags.as<uint64_t>(), s);
    scan(ws, flags.as<uint64_t>(), rank.as<uint64_t>(), domain, s);
    HIP_CHECK(hipGetLastError());
    const uint64_t items = read_value(rank.as<uint64_t>() + domain, s);
    ws->graph_text.items.reserve(std::max<uint64_t>(items, 1) * sizeof(uint64_t));
    ws->graph_text.soff.reserve((items + 1) * sizeof(uint64_t));
    sizes.reserve(std::max<uint64_t>(items, 1) * sizeof(uint64_t));
    launch_scatter_ids(rank.as<uint64_t>(), domain, translated ? 0 : g.min_node, ws->graph_text.items.as<uint64_t>(), s);
    launch_segment_line_sizes(t, ws->graph_text.items.as<uint64_t>(), items, translated, sizes.as<uint64_t>(), s);
    scan(ws, sizes.as<uint64_t>(), ws->graph_text.soff.as<uint64_t>(), items, s);
    // 2. the edge rows of every (node | segment, orientation), with the row of every edge
    ids.reserve(std::max<uint64_t>(queries, 1) * sizeof(uint64_t));
    orient.reserve(std::max<uint64_t>(queries, 1));
    counts.reserve(std::max<uint64_t>(queries, 1) * sizeof(uint64_t));
    off.reserve((queries + 1) * sizeof(uint64_t));
    valid.reserve(std::max<uint64_t>(queries, 1));
    big.reserve((queries + 1) * sizeof(uint32_t));
    if (translated) launch_link_queries(t, nullptr, nullptr, queries, false, ids.as<uint64_t>(), orient.as<uint8_t>(), s);
    else launch_all_node_queries(g, ids.as<uint64_t>(), orient.as<uint8_t>(), s);
    launch_edge_count(ix->dev, ids.as<uint64_t>(), orient.as<uint8_t>(), queries, false, counts.as<uint64_t>(), valid.as<uint8_t>(), s);
    scan(ws, counts.as<uint64_t>(), off.as<uint64_t>(), queries, s);
    HIP_CHECK(hipGetLastError());
    const uint64_t sbytes = read_value(ws->graph_text.soff.as<uint64_t>() + items, s);
    const uint64_t edges = read_value(off.as<uint64_t>() + queries, s);
    ws->graph_text.edges.reserve(std::max<uint64_t>(edges, 1) * sizeof(uint64_t));
    ws->graph_text.rows.reserve(std::max<uint64_t>(edges, 1) * sizeof(uint32_t));
    ws->graph_text.loff.reserve((edges + 1) * sizeof(uint64_t));
    launch_edge_fill(ix->dev, ids.as<uint64_t>(), orient.as<uint8_t>(), queries, false, off.as<uint64_t>(), ws->graph_text.edges.as<uint64_t>(), ws->graph_text.rows.as<uint32_t>(),
                     big.as<uint32_t>(), s);
    // 3. the sizes of the L-lines: with a translation a row ends at its first node without a segment (LinkIter)
    if (translated) {
        cut.reserve(std::max<uint64_t>(queries, 1) * sizeof(uint64_t));
        launch_link_cut(t, off.as<uint64_t>(), ws->graph_text.edges.as<uint64_t>(), ws->graph_text.rows.as<uint32_t>(), queries, edges, cut.as<uint64_t>(), s);
    }
    sizes.reserve(std::max<uint64_t>(edges, 1) * sizeof(uint64_t));
    lines.reserve(sizeof(uint64_t));
    HIP_CHECK(hipMemsetAsync(lines.ptr, 0, sizeof(uint64_t), s));
    launch_link_line_sizes(t, g, translated, off.as<uint64_t>(), ws->graph_text.edges.as<uint64_t>(), ws->graph_text.rows.as<uint32_t>(), edges, translated ? cut.as<uint64_t>() : nullptr,
                           sizes.as<uint64_t>(), lines.as<uint64_t>(), s);
    scan(ws, sizes.as<uint64_t>(), ws->graph_text.loff.as<uint64_t>(), edges, s);
    HIP_CHECK(hipGetLastError());
    ws->graph_text.lbytes = read_value(ws->graph_text.loff.as<uint64_t>() + edges, s);
    ws->graph_text.links = read_value(lines.as<uint64_t>(), s);
    ws->graph_text.item_count = items; ws->graph_text.edge_count = edges; ws->graph_text.sbytes = sbytes; ws->graph_text.translated = translated;
    ws->graph_text.sized = true;                                   // (the scratch buffers go here: hipFree waits for the stream)
}

gbwt_hip_status graph_lines_compute(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, bool format_again) {
    if (!ix || !ws || ws->index != ix) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    if (!ix->host.is_gbz || !(ix->caps & GBWT_HIP_OPEN_GFA)) return fail(GBWT_HIP_BAD_ARGUMENT, NEEDS_GFA);
    if (ws->graph_text.text_valid && !format_again) return GBWT_HIP_OK;
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        ensure_labels(ix);
        hipStream_t s = ws->stream;
        ws->graph_text.ev.ensure();
        const GraphTables t = graph_tables(ix, true);
        const ComponentGeometry g = graph_geometry(ix->dev);
        ws->graph_text.text_valid = false;
        ws->graph_text.timed = false;
        HIP_CHECK(hipEventRecord(ws->graph_text.ev[0], s));
        ws->graph_text.sized_now = !ws->graph_text.sized;
        if (!ws->graph_text.sized) graph_lines_size(ix, ws, t, g, s);
        HIP_CHECK(hipEventRecord(ws->graph_text.ev[1], s));
        const uint64_t head = ws->graph_text.header.size();
        ws->graph_text.text.reserve(head + ws->graph_text.sbytes + ws->graph_text.lbytes + 16);
        HIP_CHECK(hipMemcpyAsync(ws->graph_text.text.ptr, ws->graph_text.header.data(), head, hipMemcpyHostToDevice, s));
        launch_segment_lines(t, ws->graph_text.items.as<uint64_t>(), ws->graph_text.item_count, ws->graph_text.translated, ws->graph_text.soff.as<uint64_t>(), head, ws->graph_text.sbytes, ws->graph_text.text.as<char>(), s);
        HIP_CHECK(hipEventRecord(ws->graph_text.ev[2], s));
        launch_link_lines(t, g, ws->graph_text.translated, ws->graph_text.edges.as<uint64_t>(), ws->graph_text.rows.as<uint32_t>(), ws->graph_text.edge_count, ws->graph_text.loff.as<uint64_t>(), head + ws->graph_text.sbytes,
                          ws->graph_text.text.as<char>(), s);
        HIP_CHECK(hipEventRecord(ws->graph_text.ev[3], s));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        ws->graph_text.text_valid = true;
        ws->graph_text.timed = true;
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const HipError &e) {
        return status_of(e);
    }
}

// Graph::node_to_segment (src/graph.rs:186-198) behind GBZ::node_to_segment's tests (src/gbz.rs:370-376)
bool host_segment_of(const HostIndex &h, uint64_t node_id, uint64_t &segment) {
    if (!h.is_gbz || !h.has_translation || h.segment_starts.empty()) return false;
    if (node_id >= h.mapping_len || node_id < h.segment_starts[0] || !node_exists(h, node_id)) return false;
    segment = static_cast<uint64_t>(std::upper_bound(h.segment_starts.begin(), h.segment_starts.end(), node_id) - h.segment_starts.begin()) - 1;
    return true;
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_node_ids(const gbwt_hip_index *ix, uint64_t *out, uint64_t capacity, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !total) return fail(GBWT_HIP_BAD_ARGUMENT, "null index / total");
    *total = 0;
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        const ComponentGeometry g = graph_geometry(ix->dev);
        if (g.slots == 0) return GBWT_HIP_OK;
        DeviceBuffer flags, rank, temp, ids;
        const size_t temp_bytes = scan_temp_bytes(g.slots);
        flags.reserve(g.slots * sizeof(uint64_t));
        rank.reserve((g.slots + 1) * sizeof(uint64_t));
        temp.reserve(temp_bytes);
        launch_node_flags(ix->dev, g, flags.as<uint64_t>(), nullptr);
        launch_scan(flags.as<uint64_t>(), rank.as<uint64_t>(), g.slots, temp.ptr, temp_bytes, nullptr);
        HIP_CHECK(hipGetLastError());
        *total = read_value(rank.as<uint64_t>() + g.slots, nullptr);
        if (!out) return GBWT_HIP_OK;
        if (capacity < *total) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the node ids");
        if (*total == 0) return GBWT_HIP_OK;
        ids.reserve(*total * sizeof(uint64_t));
        launch_scatter_ids(rank.as<uint64_t>(), g.slots, g.min_node, ids.as<uint64_t>(), nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out, ids.ptr, *total * sizeof(uint64_t), hipMemcpyDeviceToHost));
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_edges(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *node_ids, const uint8_t *orientations, uint64_t n, int predecessors,
                               uint64_t *out_offsets, uint64_t *out_edges, uint64_t capacity, uint64_t *total, uint8_t *valid) {
    GBWT_HIP_GUARD_BEGIN
    return rows_to_host(ix, ws, node_ids, orientations, n, predecessors, 0, out_offsets, out_edges, capacity, total, valid);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_edges_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *node_ids, const uint8_t *orientations, uint64_t n, int predecessors,
                                      gbwt_hip_edge_rows *out) {
    GBWT_HIP_GUARD_BEGIN
    return rows_device(ix, ws, node_ids, orientations, n, predecessors, 0, out);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_links(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *segment_ids, const uint8_t *orientations, uint64_t n, int predecessors,
                               uint64_t *out_offsets, uint64_t *out_links, uint64_t capacity, uint64_t *total, uint8_t *valid) {
    GBWT_HIP_GUARD_BEGIN
    return rows_to_host(ix, ws, segment_ids, orientations, n, predecessors, 1, out_offsets, out_links, capacity, total, valid);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_links_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *segment_ids, const uint8_t *orientations, uint64_t n, int predecessors,
                                      gbwt_hip_edge_rows *out) {
    GBWT_HIP_GUARD_BEGIN
    return rows_device(ix, ws, segment_ids, orientations, n, predecessors, 1, out);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_segments(const gbwt_hip_index *ix, uint64_t *out_ids, uint64_t capacity, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !total) return fail(GBWT_HIP_BAD_ARGUMENT, "null index / total");
    *total = 0;
    const HostIndex &h = ix->host;
    if (!h.is_gbz) return fail(GBWT_HIP_BAD_ARGUMENT, "segments need a GBZ, this handle holds a bare GBWT");
    if (!h.has_translation) return GBWT_HIP_OK;
    std::vector<uint64_t> ids;
    for (uint64_t s = 0; s < h.segment_starts.size(); s++)
        if (node_exists(h, h.segment_starts[s])) ids.push_back(s);
    *total = ids.size();
    if (!out_ids) return GBWT_HIP_OK;
    if (capacity < ids.size()) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the segments");
    std::copy(ids.begin(), ids.end(), out_ids);
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_node_segments(const gbwt_hip_index *ix, const uint64_t *node_ids, uint64_t n, uint64_t *out_segments, uint8_t *valid) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || (n && (!node_ids || !out_segments || !valid))) return fail(GBWT_HIP_BAD_ARGUMENT, "null index / node_ids / output");
    if (!ix->host.is_gbz) return fail(GBWT_HIP_BAD_ARGUMENT, "segments need a GBZ, this handle holds a bare GBWT");
    for (uint64_t k = 0; k < n; k++) {
        out_segments[k] = 0;
        valid[k] = host_segment_of(ix->host, node_ids[k], out_segments[k]) ? 1 : 0;
    }
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_graph_lines_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, gbwt_hip_graph_text *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_graph_text{nullptr, 0, 0, 0, 0, 0};
    const gbwt_hip_status st = graph_lines_compute(ix, ws, true);
    if (st != GBWT_HIP_OK) return st;
    *out = gbwt_hip_graph_text{ws->graph_text.text.as<char>(), ws->graph_text.header.size(), ws->graph_text.sbytes, ws->graph_text.lbytes, ws->graph_text.item_count, ws->graph_text.links};
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_graph_lines(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, char *out, uint64_t capacity, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (!total) return fail(GBWT_HIP_BAD_ARGUMENT, "null total");
    *total = 0;
    const gbwt_hip_status st = graph_lines_compute(ix, ws, false);
    if (st != GBWT_HIP_OK) return st;
    *total = ws->graph_text.header.size() + ws->graph_text.sbytes + ws->graph_text.lbytes;
    if (!out) return GBWT_HIP_OK;
    if (capacity < *total) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the graph lines");
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        copy_to_host(ws, out, ws->graph_text.text.ptr, *total);
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_graph_ms(const gbwt_hip_workspace *ws, float *size_ms, float *segments_ms, float *links_ms) {
    GBWT_HIP_GUARD_BEGIN
    if (!ws || !ws->graph_text.timed) return fail(GBWT_HIP_BAD_ARGUMENT, "no timed graph lines request on this workspace");
    float ms[3] = {0, 0, 0};
    for (int k = 0; k < 3; k++)
        if (hipEventElapsedTime(&ms[k], ws->graph_text.ev[k], ws->graph_text.ev[k + 1]) != hipSuccess) return fail(GBWT_HIP_DEVICE_ERROR, "hipEventElapsedTime failed");
    if (size_ms) *size_ms = ws->graph_text.sized_now ? ms[0] : 0.0f;
    if (segments_ms) *segments_ms = ms[1];
    if (links_ms) *links_ms = ms[2];
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

}  // extern "C"
