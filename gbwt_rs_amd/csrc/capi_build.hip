// capi_build.hip -- GBWT construction over the C ABI (include/gbwt_hip.h, "construction"): the checks of a path set, the records made by
// build.hip, the open behind them, and the two entry points that give a handle's records back: gbwt_hip_records and gbwt_hip_save.
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "build.hpp"
#include "build_codec.hpp"
#include "capi_internal.hpp"
#include "hip_raii.hpp"

using namespace gbwt_hip;

namespace {

gbwt_hip_status check_call(const void *offsets, uint64_t n_paths, int bidirectional, uint32_t flags, gbwt_hip_index **out) {
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = nullptr;
    if (n_paths && !offsets) return fail(GBWT_HIP_BAD_ARGUMENT, "null offsets");
    if (bidirectional != 0 && bidirectional != 1) return fail(GBWT_HIP_BAD_ARGUMENT, "bidirectional must be 0 or 1");
    return check_open_flags(flags);
}

}  // namespace

namespace gbwt_hip {

// sizes the construction counts in 32 bits (also the check of a construction from GFA, capi_gfa_build.hip)
gbwt_hip_status check_build_sizes(uint64_t n_paths, uint64_t path_visits, int bidirectional) {
    const uint64_t limit = BUILD_MAX_SLOTS >> bidirectional;
    if (n_paths > limit || path_visits > limit || n_paths + path_visits > limit)
        return fail(GBWT_HIP_UNSUPPORTED, std::to_string(path_visits) + " visits + " + std::to_string(n_paths) + " sequences" + (bidirectional ? ", twice in a bidirectional index" : "") +
                                              ": more than 2^32 - 1 are not supported (u32 positions on device)");
    return GBWT_HIP_OK;
}

gbwt_hip_status check_build_range(uint64_t min_node, uint64_t max_node) {
    if (max_node > 0xFFFFFFFFull) return fail(GBWT_HIP_UNSUPPORTED, "alphabet_size > 2^32 is not supported (u32 node ids on device)");
    if (max_node + 1 - (min_node - 1) >= BUILD_MAX_RECORDS) return fail(GBWT_HIP_UNSUPPORTED, "more than 2^30 records are not supported");
    return GBWT_HIP_OK;
}

// The index of a set without visits: the endmarker's record alone -- every sequence ends where it starts
void build_without_visits(uint64_t sequences, BuildOutput &o) {
    o.sequences = sequences; o.visits = 0; o.records = 1; o.alphabet_offset = 0; o.alphabet_size = 1;
    uint8_t bytes[32], *p = bytes;
    if (sequences == 0) p = build_codec::write_header(p, 0);
    else p = build_codec::write_run(build_codec::write_edge(build_codec::write_header(p, 1), 0, 0), 1, 0, sequences);
    o.data.assign(bytes, p);
    o.starts.assign(1, 0);
}

std::unique_ptr<gbwt_hip_index> handle_from_build(const BuildOutput &o, bool bidirectional, int device, uint32_t flags) {
    std::unique_ptr<gbwt_hip_index> ix = new_handle(device, flags);
    ix->host = index_from_records(o.data.data(), o.data.size(), o.starts.data(), o.starts.size(), o.alphabet_offset, o.alphabet_size, o.sequences, o.visits + o.sequences, bidirectional);
    return ix;
}

}  // namespace gbwt_hip

namespace {

// offsets on the host: a CSR, and sizes the construction counts in 32 bits
gbwt_hip_status check_offsets(const uint64_t *offsets, uint64_t n_paths, int bidirectional, uint64_t &path_visits) {
    path_visits = 0;
    if (n_paths == 0) return GBWT_HIP_OK;
    if (offsets[0] != 0) return fail(GBWT_HIP_BAD_ARGUMENT, "offsets must start at 0 (offsets[0] = " + std::to_string(offsets[0]) + ")");
    for (uint64_t p = 0; p < n_paths; p++)
        if (offsets[p + 1] < offsets[p]) return fail(GBWT_HIP_BAD_ARGUMENT, "offsets decrease at path " + std::to_string(p));
    path_visits = offsets[n_paths];
    return check_build_sizes(n_paths, path_visits, bidirectional);
}

// d_offsets / d_nodes in HBM of `device` (made current by the caller), the range of the nodes over the sequences known
gbwt_hip_status build_and_open(const uint64_t *d_offsets, const uint32_t *d_nodes, uint64_t n_paths, uint64_t path_visits, uint64_t min_node, uint64_t max_node, int bidirectional,
                               int device, uint32_t flags, hipStream_t s, gbwt_hip_index **out) {
    BuildOutput o;
    if (path_visits == 0) build_without_visits(n_paths << bidirectional, o);
    else {
        const BuildInput in{d_offsets, d_nodes, n_paths, path_visits, bidirectional != 0, min_node, max_node};
        build_records_on_device(in, o, s);               // (all of its scratch is free again when it returns)
    }
    const auto t_open = Clock::now();
    const gbwt_hip_status st = open_host_index(handle_from_build(o, bidirectional != 0, device, flags), out, t_open);
    if (st != GBWT_HIP_OK) return st;
    (*out)->build_info = build_info_of(o);
    (*out)->build_info.open_ms = ms_since(t_open);
    return GBWT_HIP_OK;
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_build_from_paths(const uint64_t *offsets, const uint64_t *nodes, uint64_t n_paths, int bidirectional, int device, uint32_t flags, gbwt_hip_index **out) {
    GBWT_HIP_GUARD_BEGIN
    gbwt_hip_status st = check_call(offsets, n_paths, bidirectional, flags, out);
    if (st != GBWT_HIP_OK) return st;
    uint64_t path_visits = 0;
    st = check_offsets(offsets, n_paths, bidirectional, path_visits);
    if (st != GBWT_HIP_OK) return st;
    if (path_visits && !nodes) return fail(GBWT_HIP_BAD_ARGUMENT, "null nodes");
    uint64_t min_node = ~uint64_t(0), max_node = 0;
    for (uint64_t k = 0; k < path_visits; k++) {
        if (nodes[k] < 2) return fail(GBWT_HIP_BAD_ARGUMENT, "node " + std::to_string(nodes[k]) + " at position " + std::to_string(k) + " is below 2 (a node is 2 * id + orientation, id >= 1)");
        min_node = std::min(min_node, nodes[k]); max_node = std::max(max_node, nodes[k]);
    }
    if (path_visits) {
        if (bidirectional) { min_node &= ~uint64_t(1); max_node |= 1; }   // the reverse sequences visit the flipped nodes
        st = check_build_range(min_node, max_node);
        if (st != GBWT_HIP_OK) return st;
    }
    st = require_device();
    if (st != GBWT_HIP_OK) return st;
    try {
        HIP_CHECK(hipSetDevice(device));
        Stream stream;
        DeviceBuffer d_offsets, d_nodes;
        if (path_visits) {
            std::vector<uint32_t> narrow(path_visits);
            for (uint64_t k = 0; k < path_visits; k++) narrow[k] = static_cast<uint32_t>(nodes[k]);
            d_offsets.reserve((n_paths + 1) * sizeof(uint64_t));
            d_nodes.reserve(path_visits * sizeof(uint32_t));
            HIP_CHECK(hipMemcpyAsync(d_offsets.ptr, offsets, (n_paths + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream.s));
            HIP_CHECK(hipMemcpyAsync(d_nodes.ptr, narrow.data(), path_visits * sizeof(uint32_t), hipMemcpyHostToDevice, stream.s));
            HIP_CHECK(hipStreamSynchronize(stream.s));   // (`narrow` goes out of scope)
        }
        return build_and_open(d_offsets.as<uint64_t>(), d_nodes.as<uint32_t>(), n_paths, path_visits, min_node, max_node, bidirectional, device, flags, stream.s, out);
    } catch (const HipError &e) {
        return status_of(e, "the construction");
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_build_from_rows_device(const uint64_t *d_offsets, const uint32_t *d_nodes, uint64_t n_paths, int bidirectional, int device, uint32_t flags,
                                                gbwt_hip_index **out) {
    GBWT_HIP_GUARD_BEGIN
    gbwt_hip_status st = check_call(d_offsets, n_paths, bidirectional, flags, out);
    if (st != GBWT_HIP_OK) return st;
    st = require_device();
    if (st != GBWT_HIP_OK) return st;
    try {
        HIP_CHECK(hipSetDevice(device));
        Stream stream;
        std::vector<uint64_t> offsets(n_paths + 1, 0);
        if (n_paths) HIP_CHECK(hipMemcpy(offsets.data(), d_offsets, (n_paths + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        uint64_t path_visits = 0;
        st = check_offsets(offsets.data(), n_paths, bidirectional, path_visits);
        if (st != GBWT_HIP_OK) return st;
        if (path_visits && !d_nodes) return fail(GBWT_HIP_BAD_ARGUMENT, "null nodes");
        uint64_t min_node = 0, max_node = 0;
        if (path_visits) {
            uint32_t lo = 0, hi = 0;
            build_node_range(d_nodes, path_visits, lo, hi, stream.s);
            if (lo < 2) return fail(GBWT_HIP_BAD_ARGUMENT, "a node of the rows is " + std::to_string(lo) + ", below 2 (a node is 2 * id + orientation, id >= 1)");
            min_node = lo; max_node = hi;
            if (bidirectional) { min_node &= ~uint64_t(1); max_node |= 1; }
            st = check_build_range(min_node, max_node);
            if (st != GBWT_HIP_OK) return st;
        }
        return build_and_open(d_offsets, d_nodes, n_paths, path_visits, min_node, max_node, bidirectional, device, flags, stream.s, out);
    } catch (const HipError &e) {
        return status_of(e, "the construction");
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_records(const gbwt_hip_index *ix, uint8_t *out_data, uint64_t data_capacity, uint64_t *data_len, uint64_t *out_starts, uint64_t starts_capacity,
                                 uint64_t *n_records) {
    GBWT_HIP_GUARD_BEGIN
    if (data_len) *data_len = 0;
    if (n_records) *n_records = 0;
    if (!ix || !data_len || !n_records) return fail(GBWT_HIP_BAD_ARGUMENT, "null index / data_len / n_records");
    ix->host.ensure_records();
    const HostIndex &h = ix->host;
    const uint64_t records = h.starts.empty() ? 0 : h.starts.size() - 1;
    *data_len = h.data.size();
    *n_records = records;
    if (!out_data && !out_starts) return GBWT_HIP_OK;
    if ((*data_len && !out_data) || (records && !out_starts)) return fail(GBWT_HIP_BAD_ARGUMENT, "null buffer");
    if (data_capacity < *data_len || starts_capacity < records) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the records");
    if (*data_len) std::memcpy(out_data, h.data.data(), *data_len);
    if (records) std::memcpy(out_starts, h.starts.data(), records * sizeof(uint64_t));
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_save(const gbwt_hip_index *ix, const char *path) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !path) return fail(GBWT_HIP_BAD_ARGUMENT, "null index / path");
    ix->host.ensure_records();
    save_index_file(ix->host, path, ix->host.is_gbz);
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_build_info(const gbwt_hip_index *ix, gbwt_hip_build_info *out) {
    GBWT_HIP_GUARD_BEGIN
    return last_info(ix, out, &gbwt_hip_index::build_info);
    GBWT_HIP_GUARD_END
}

}  // extern "C"
