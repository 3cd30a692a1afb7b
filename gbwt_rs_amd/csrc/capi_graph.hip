// capi_graph.hip -- graph topology over the C ABI: the weakly connected components of a handle (GBZ::weakly_connected_components,
// src/gbz.rs:570-598), made on first use from the record bytes, the record starts and the endmarker in HBM (components.hip), and
// gbz-extract's contig path selection on top of them (select_paths, src/bin/gbz-extract.rs:196-264).
#include <string>
#include <vector>

#include "capi_internal.hpp"
#include "scan.hpp"

using namespace gbwt_hip;

namespace {

// stream, events and the pinned word of one build
struct BuildScratch {
    Stream stream;
    EventSet<2> ev;
    uint32_t *pinned = nullptr;
    BuildScratch() { HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&pinned), 4 * sizeof(uint32_t))); }
    BuildScratch(const BuildScratch &) = delete;
    BuildScratch &operator=(const BuildScratch &) = delete;
    ~BuildScratch() {
        (void)hipStreamSynchronize(stream);
        if (pinned) (void)hipHostFree(pinned);
    }
    void begin() { HIP_CHECK(hipEventRecord(ev[0], stream)); }
    // waits for the stream; milliseconds since begin()
    float end() {
        HIP_CHECK(hipEventRecord(ev[1], stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipGetLastError());
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        return ms;
    }
};

// The components of a handle, made once by the first call that needs them (any thread).  A failure marks nothing: the next call tries again.
void ensure_components(const gbwt_hip_index *ix) {
    ix->components.built.ensure([ix]() {
        HIP_CHECK(hipSetDevice(ix->device));
        const DeviceIndex &d = ix->dev;
        ComponentGeometry g{0, 0};
        if (d.n_records > 1) {
            g.min_node = d.first_node >> 1;                                                    // GBZ::min_node = node_id(first_node)
            g.slots = ((static_cast<uint64_t>(d.alphabet_offset) + d.n_records - 1) >> 1) - g.min_node + 1;   // GBZ::max_node = node_id(alphabet_size) - 1
        }
        if (g.slots > 0x7FFFFFFFull) throw Unsupported("too many node slots for the components (32-bit labels)");
        const uint64_t slots = g.slots, stride = ix->host.bidirectional ? 2 : 1, paths = d.n_sequences / stride;
        gbwt_hip_components_times times{};
        BuildScratch b;
        DeviceBuffer changed;
        changed.reserve(sizeof(uint32_t));
        ix->components.of.reserve(std::max<uint64_t>(slots, 4) * sizeof(uint32_t));
        uint32_t *label = ix->components.of.as<uint32_t>();
        // 1. labels: hook passes over the records, jump passes over the labels in between, until a hook pass changes nothing
        const auto pass = [&](bool hook) {
            HIP_CHECK(hipMemsetAsync(changed.ptr, 0, sizeof(uint32_t), b.stream));
            b.begin();
            if (hook) launch_component_hook(d, g, label, changed.as<uint32_t>(), b.stream);
            else launch_component_jump(label, slots, changed.as<uint32_t>(), b.stream);
            HIP_CHECK(hipMemcpyAsync(b.pinned, changed.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream));
            const float ms = b.end();
            if (hook) { times.hook_ms += ms; times.hook_launches++; } else { times.jump_ms += ms; times.jump_launches++; }
            return b.pinned[0] != 0;
        };
        launch_component_init(label, slots, b.stream);
        while (slots != 0 && pass(true))
            while (pass(false)) {}
        // 2. component numbers, CSR, path components
        uint64_t components = 0, nodes = 0;
        ix->components.paths.reserve(std::max<uint64_t>(paths, 4) * sizeof(uint32_t));
        b.begin();
        if (slots != 0) {
            DeviceBuffer first, flag, rank, key, value, temp, counts;
            ComponentShape w{};
            w.temp_bytes = std::max<size_t>(component_shape_temp_bytes(slots), 16);
            for (DeviceBuffer *q : {&first, &flag, &rank, &key, &value}) q->reserve(slots * sizeof(uint32_t));
            temp.reserve(w.temp_bytes);
            w.label = label; w.first = first.as<uint32_t>(); w.flag = flag.as<uint32_t>(); w.rank = rank.as<uint32_t>(); w.key = key.as<uint32_t>();
            w.value = value.as<uint32_t>(); w.temp = temp.ptr;
            launch_component_numbers(d, g, w, b.stream);
            HIP_CHECK(hipMemcpyAsync(b.pinned, w.rank + (slots - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream));
            HIP_CHECK(hipMemcpyAsync(b.pinned + 1, w.flag + (slots - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream));
            HIP_CHECK(hipStreamSynchronize(b.stream));
            components = static_cast<uint64_t>(b.pinned[0]) + b.pinned[1];
            times.shape_launches += 5;
            ix->components.offsets.reserve((components + 1) * sizeof(uint64_t));
            counts.reserve(std::max<uint64_t>(components, 1) * sizeof(uint64_t));
            DeviceBuffer scan_temp;
            const size_t tb = scan_temp_bytes(components);
            scan_temp.reserve(tb);
            launch_component_counts(g, label, components, counts.as<uint64_t>(), b.stream);
            launch_scan(counts.as<uint64_t>(), ix->components.offsets.as<uint64_t>(), components, scan_temp.ptr, tb, b.stream);
            uint64_t *total = reinterpret_cast<uint64_t *>(b.pinned + 2);
            HIP_CHECK(hipMemcpyAsync(total, ix->components.offsets.as<uint64_t>() + components, sizeof(uint64_t), hipMemcpyDeviceToHost, b.stream));
            HIP_CHECK(hipStreamSynchronize(b.stream));
            nodes = *total;
            ix->components.nodes.reserve(std::max<uint64_t>(nodes, 4) * sizeof(uint32_t));
            launch_component_csr(g, w, components, ix->components.nodes.as<uint32_t>(), b.stream);
            times.shape_launches += 4;
            launch_path_components(d, g, label, paths, static_cast<uint32_t>(stride), ix->components.paths.as<uint32_t>(), b.stream);
            times.shape_launches += paths ? 1 : 0;
            ix->components.host_paths.assign(paths, COMPONENT_NONE);
            if (paths) HIP_CHECK(hipMemcpyAsync(ix->components.host_paths.data(), ix->components.paths.ptr, paths * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream));
            times.shape_ms = b.end();                       // (before the scratch buffers go: hipFree waits anyway)
        } else {
            ix->components.offsets.reserve(sizeof(uint64_t));
            ix->components.nodes.reserve(sizeof(uint32_t));
            HIP_CHECK(hipMemsetAsync(ix->components.offsets.ptr, 0, sizeof(uint64_t), b.stream));
            if (paths) HIP_CHECK(hipMemsetAsync(ix->components.paths.ptr, 0xFF, paths * sizeof(uint32_t), b.stream));
            ix->components.host_paths.assign(paths, COMPONENT_NONE);
            times.shape_ms = b.end();
        }
        ix->components.geometry = g;
        ix->components.count = components;
        ix->components.node_count = nodes;
        ix->components.times = times;
    });
}

// select_paths (src/bin/gbz-extract.rs:196-264); throws InvalidData with the reference's messages
std::vector<uint64_t> select_paths(const gbwt_hip_index *ix, const char *contig) {
    const HostIndex &h = ix->host;
    if (!h.has_metadata) throw InvalidData("Sequence extraction requires GBWT metadata");
    if (!(h.metadata_flags & 1) || h.path_names.empty()) throw InvalidData("Sequence extraction requires path names");
    std::vector<uint64_t> selected;
    if (!contig) {
        for (uint64_t p = 0; p < h.path_names.size(); p++) selected.push_back(p);       // 0..metadata.paths()
        return selected;
    }
    const std::string name(contig);
    if (!(h.metadata_flags & 4)) throw InvalidData("Cannot select a contig without contig names");
    uint64_t contig_id = 0;
    if (!h.contig_names.find(name, contig_id)) throw InvalidData("The graph does not contain contig " + name);
    std::vector<uint64_t> initial;
    for (uint64_t p = 0; p < h.path_names.size(); p++)
        if (h.path_names[p].contig == contig_id) initial.push_back(p);
    if (initial.empty()) throw InvalidData("The graph does not contain any paths for contig " + name);
    ensure_components(ix);
    const std::vector<uint32_t> &of = ix->components.host_paths;
    std::vector<uint8_t> wanted(ix->components.count, 0);
    for (uint64_t p : initial)
        if (p < of.size() && of[p] != COMPONENT_NONE) wanted[of[p]] = 1;
    for (uint64_t p = 0; p < of.size(); p++)                                             // 0..gbz.paths()
        if (of[p] != COMPONENT_NONE && wanted[of[p]]) selected.push_back(p);
    return selected;
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_components_device(const gbwt_hip_index *ix, gbwt_hip_components *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !out) return fail(GBWT_HIP_BAD_ARGUMENT, "null index / output");
    *out = gbwt_hip_components{};
    try {
        ensure_components(ix);
    } catch (const HipError &e) {
        return status_of(e);
    }
    out->d_component = ix->components.of.as<uint32_t>();
    out->d_offsets = ix->components.offsets.as<uint64_t>();
    out->d_nodes = ix->components.nodes.as<uint32_t>();
    out->d_path_component = ix->components.paths.as<uint32_t>();
    out->min_node = ix->components.geometry.min_node;
    out->slots = ix->components.geometry.slots;
    out->components = ix->components.count;
    out->nodes = ix->components.node_count;
    out->paths = ix->components.host_paths.size();
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

// GBZ::weakly_connected_components (src/gbz.rs:570-598) as a host CSR
gbwt_hip_status gbwt_hip_weakly_connected_components(const gbwt_hip_index *ix, uint64_t *out_offsets, uint64_t offsets_capacity, uint64_t *out_nodes, uint64_t nodes_capacity,
                                                     uint64_t *components, uint64_t *nodes) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !components || !nodes) return fail(GBWT_HIP_BAD_ARGUMENT, "null index / components / nodes");
    *components = 0; *nodes = 0;
    try {
        ensure_components(ix);
        *components = ix->components.count;
        *nodes = ix->components.node_count;
        if (!out_offsets && !out_nodes) return GBWT_HIP_OK;
        if ((out_offsets && offsets_capacity < ix->components.count + 1) || (out_nodes && nodes_capacity < ix->components.node_count))
            return fail(GBWT_HIP_CAPACITY, "output capacity too small for the components");
        HIP_CHECK(hipSetDevice(ix->device));
        if (out_offsets) HIP_CHECK(hipMemcpy(out_offsets, ix->components.offsets.ptr, (ix->components.count + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (out_nodes && ix->components.node_count) {
            std::vector<uint32_t> ids(ix->components.node_count);
            HIP_CHECK(hipMemcpy(ids.data(), ix->components.nodes.ptr, ids.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (size_t k = 0; k < ids.size(); k++) out_nodes[k] = ids[k];
        }
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

// the component of the first node of every path (select_paths, src/bin/gbz-extract.rs:243-246)
gbwt_hip_status gbwt_hip_path_components(const gbwt_hip_index *ix, const uint64_t *path_ids, uint64_t n, uint32_t *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || (n && (!path_ids || !out))) return fail(GBWT_HIP_BAD_ARGUMENT, "null index / path_ids / output");
    try {
        ensure_components(ix);
    } catch (const HipError &e) {
        return status_of(e);
    }
    const std::vector<uint32_t> &of = ix->components.host_paths;
    for (uint64_t k = 0; k < n; k++)
        if (path_ids[k] >= of.size()) return fail(GBWT_HIP_BAD_ARGUMENT, "path id out of range");
    for (uint64_t k = 0; k < n; k++) out[k] = of[path_ids[k]];
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_components_ms(const gbwt_hip_index *ix, gbwt_hip_components_times *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !out) return fail(GBWT_HIP_BAD_ARGUMENT, "null index / output");
    if (!ix->components.built.made()) return fail(GBWT_HIP_BAD_ARGUMENT, "the components of this handle have not been made yet");
    *out = ix->components.times;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

// select_paths of gbz-extract (src/bin/gbz-extract.rs:196-264)
gbwt_hip_status gbwt_hip_select_paths(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const char *contig, uint64_t *out_path_ids, uint64_t capacity, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !ws || ws->index != ix || !total) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace / total");
    *total = 0;
    try {
        const std::vector<uint64_t> selected = select_paths(ix, contig);
        *total = selected.size();
        if (!out_path_ids) return GBWT_HIP_OK;
        if (capacity < selected.size()) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the selected paths");
        std::copy(selected.begin(), selected.end(), out_path_ids);
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

// gbz-extract -c contig -o path (extract_sequences, src/bin/gbz-extract.rs:266-294)
gbwt_hip_status gbwt_hip_write_sequences_contig(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const char *path, const char *contig, int endmarker) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !ws || ws->index != ix || !path) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace / path");
    std::vector<uint64_t> selected;
    try {
        selected = select_paths(ix, contig);
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const HipError &e) {
        return status_of(e);
    }
    selected.reserve(1);                                   // (an empty selection is not NULL = all paths)
    return gbwt_hip_write_sequences(ix, ws, path, selected.data(), selected.size(), endmarker);
    GBWT_HIP_GUARD_END
}

}  // extern "C"
