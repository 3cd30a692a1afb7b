// capi_remove.hip -- GBWT / GBZ path removal over the C ABI (include/gbwt_hip.h, "removal"): the checks of the handle and the path ids, the
// records by deletion (remove.hip) or by a construction over the extracted rows of the kept sequences (build.hip), the metadata, tags and
// labels of remove_meta.hpp, and the open behind them.
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "build.hpp"
#include "capi_internal.hpp"
#include "hip_raii.hpp"
#include "merge.hpp"
#include "remove.hpp"
#include "remove_meta.hpp"

using namespace gbwt_hip;

namespace {

// REMOVE_REBUILD: the rows of the kept sequences through the construction -- as sequences, so the order is kept exactly
gbwt_hip_status rebuild(const gbwt_hip_index *ix, const std::vector<uint64_t> &kept, BuildOutput &o, hipStream_t s) {
    Workspace w;
    gbwt_hip_paths rows;
    gbwt_hip_status st = extract_rows(ix, w, kept.data(), kept.size(), rows);
    if (st != GBWT_HIP_OK) return st;
    if (rows.total == 0) { build_without_visits(kept.size(), o); return GBWT_HIP_OK; }
    st = check_build_sizes(rows.n, rows.total, 0);         // the widths of the construction over the kept set (known before the call where the input is within them)
    if (st != GBWT_HIP_OK) return st;
    uint32_t lo = 0, hi = 0;
    build_node_range(rows.d_nodes, rows.total, lo, hi, s);
    st = check_build_range(lo, hi);
    if (st != GBWT_HIP_OK) return st;
    build_records_on_device(BuildInput{rows.d_offsets, rows.d_nodes, rows.n, rows.total, false, lo, hi}, o, s);
    return GBWT_HIP_OK;
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_remove_paths(const gbwt_hip_index *index, const uint64_t *path_ids, uint64_t n, const gbwt_hip_remove_options *opts, uint32_t flags, gbwt_hip_index **out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = nullptr;
    if (!index) return fail(GBWT_HIP_BAD_ARGUMENT, "null index");
    if (n && !path_ids) return fail(GBWT_HIP_BAD_ARGUMENT, "null path ids");
    gbwt_hip_status st = check_open_flags(flags);
    if (st != GBWT_HIP_OK) return st;
    uint32_t algorithm = GBWT_HIP_REMOVE_AUTO;
    if (opts) {
        if (opts->algorithm > GBWT_HIP_REMOVE_DELETE) return fail(GBWT_HIP_BAD_ARGUMENT, "options: algorithm is one of GBWT_HIP_REMOVE_AUTO | _REBUILD | _DELETE");
        if (opts->reserved32 != 0 || opts->reserved[0] != 0 || opts->reserved[1] != 0) return fail(GBWT_HIP_BAD_ARGUMENT, "options: reserved must be 0");
        algorithm = opts->algorithm;
    }
    const HostIndex &hi = index->host;
    const uint64_t per_path = hi.bidirectional ? 2 : 1, paths = hi.sequences / per_path;
    std::string what;
    if (!remove_check_ids(path_ids, n, paths, what)) return fail(GBWT_HIP_BAD_ARGUMENT, what);
    const bool extractable = (index->caps & GBWT_HIP_OPEN_EXTRACT) != 0;
    if (algorithm == GBWT_HIP_REMOVE_REBUILD && !extractable) return fail(GBWT_HIP_BAD_ARGUMENT, "options: GBWT_HIP_REMOVE_REBUILD needs a handle that is open for extraction");
    // AUTO: the rebuild, which was measured faster on both shapes of tools/remove_bench.py, where it can run -- it extracts
    // the sequences --, else the deletion, which reads only what every handle keeps
    if (algorithm == GBWT_HIP_REMOVE_AUTO) algorithm = extractable ? GBWT_HIP_REMOVE_REBUILD : GBWT_HIP_REMOVE_DELETE;
    if (hi.is_gbz && hi.has_translation) return fail(GBWT_HIP_UNSUPPORTED, "remove: the graph has a node-to-segment translation: removing paths from a translated graph is not supported");

    // the paths as sequences, and the metadata without them: on the host, from what the handle holds
    const auto t_meta = Clock::now();
    std::vector<uint8_t> gone(paths, 0);
    for (uint64_t k = 0; k < n; k++) gone[path_ids[k]] = 1;
    std::vector<uint64_t> removed, kept;
    removed.reserve(n * per_path); kept.reserve(hi.sequences - n * per_path);
    for (uint64_t s = 0; s < hi.sequences; s++) (s / per_path < paths && gone[s / per_path] ? removed : kept).push_back(s);
    HostIndex meta;
    MergeRefusal bad = remove_metadata(hi, gone, meta);
    if (bad) return refusal_status(bad, "remove: ");
    meta.tags = remove_tags(hi.tags, hi.sample_names, meta.sample_names);
    meta.gbz_tags = remove_tags(hi.gbz_tags, hi.sample_names, meta.sample_names);
    double metadata_ms = ms_since(t_meta);

    // The widths of the construction (u32 positions, build.hpp).  The deletion lays out all positions of the INPUT; the rebuild those of the
    // kept sequences, whose visits the host knows only behind the extraction where the input itself is beyond the widths (rebuild()).
    const uint64_t input_visits = hi.size >= hi.sequences ? hi.size - hi.sequences : 0;
    const bool device_work = !kept.empty() && input_visits != 0;
    if (device_work) {
        st = algorithm == GBWT_HIP_REMOVE_DELETE ? check_build_sizes(hi.sequences, input_visits, 0) : check_build_sizes(kept.size(), 0, 0);
        if (st != GBWT_HIP_OK) return st;
    }

    st = require_device();
    if (st != GBWT_HIP_OK) return st;
    const int device = index->device;
    try {
        HIP_CHECK(hipSetDevice(device));
        Stream stream;
        const MergeInput in{index->dev, hi.sequences, input_visits, hi.alphabet_offset, hi.alphabet_size};
        BuildOutput o;
        RemoveWalk walk;
        if (!device_work) build_without_visits(kept.size(), o);
        else if (algorithm == GBWT_HIP_REMOVE_REBUILD) {
            st = rebuild(index, kept, o, stream.s);
            if (st != GBWT_HIP_OK) return st;
        } else remove_records_on_device(in, removed.data(), removed.size(), o, walk, stream.s);
        walk.removed_sequences = removed.size(); walk.removed_steps = in.visits - o.visits;

        const auto t_open = Clock::now();
        std::unique_ptr<gbwt_hip_index> ix = handle_from_build(o, hi.bidirectional, device, flags);
        if (hi.is_gbz) {                                   // (the graph of the nodes the new records still visit)
            const auto t_graph = Clock::now();
            bad = remove_graph(hi, ix->host, meta);
            if (bad) return refusal_status(bad, "remove: ");
            metadata_ms += ms_since(t_graph);
        }
        adopt_metadata(ix->host, std::move(meta));

        gbwt_hip_remove_info m{};
        fill_build_counters(m, o);
        m.removed_sequences = walk.removed_sequences; m.removed_steps = walk.removed_steps;
        m.algorithm_used = algorithm; m.removed = 1;
        m.walk_ms = walk.walk_ms; m.decode_ms = walk.decode_ms; m.compact_ms = walk.compact_ms;
        m.metadata_ms = metadata_ms;
        st = open_host_index(std::move(ix), out, t_open);
        if (st != GBWT_HIP_OK) return st;
        m.open_ms = ms_since(t_open);
        (*out)->remove_info = m;
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e, "the removal");
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_remove_info(const gbwt_hip_index *ix, gbwt_hip_remove_info *out) {
    GBWT_HIP_GUARD_BEGIN
    return last_info(ix, out, &gbwt_hip_index::remove_info);
    GBWT_HIP_GUARD_END
}

}  // extern "C"
