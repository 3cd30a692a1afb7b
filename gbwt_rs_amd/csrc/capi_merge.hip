// capi_merge.hip -- GBWT / GBZ merging over the C ABI (include/gbwt_hip.h, "merging"): the checks of two handles, the metadata, tags and
// labels of merge_meta.hpp, the records by insertion (merge.hip) or by a construction over the extracted rows of both (build.hip), and the
// open behind them.
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "build.hpp"
#include "capi_internal.hpp"
#include "hip_raii.hpp"
#include "merge.hpp"
#include "merge_meta.hpp"

using namespace gbwt_hip;

namespace {

MergeInput input_of(const gbwt_hip_index *ix) {
    const HostIndex &h = ix->host;
    return MergeInput{ix->dev, h.sequences, h.size - h.sequences, h.alphabet_offset, h.alphabet_size};
}

// all sequences of a handle as rows in HBM
gbwt_hip_status extract_all(const gbwt_hip_index *ix, Workspace &w, gbwt_hip_paths &rows) {
    std::vector<uint64_t> ids(ix->host.sequences);
    for (uint64_t i = 0; i < ids.size(); i++) ids[i] = i;
    return extract_rows(ix, w, ids.data(), ids.size(), rows);
}

// MERGE_REBUILD: the rows of both, behind one another, through the construction -- as sequences, so the order is kept exactly
gbwt_hip_status rebuild(const gbwt_hip_index *a, const gbwt_hip_index *b, uint64_t min_node, uint64_t max_node, BuildOutput &o, hipStream_t s) {
    Workspace wa, wb;
    gbwt_hip_paths ra, rb;
    gbwt_hip_status st = extract_all(a, wa, ra);
    if (st != GBWT_HIP_OK) return st;
    st = extract_all(b, wb, rb);
    if (st != GBWT_HIP_OK) return st;
    const uint64_t n = ra.n + rb.n, total = ra.total + rb.total;
    CountedScratch sc;
    CountedBuf offsets(sc, (n + 1) * sizeof(uint64_t)), nodes(sc, total * sizeof(uint32_t));
    merge_concat_rows(ra.d_offsets, ra.d_nodes, ra.n, ra.total, rb.d_offsets, rb.d_nodes, rb.n, rb.total, offsets.as<uint64_t>(), nodes.as<uint32_t>(), s);
    HIP_CHECK(hipStreamSynchronize(s));
    build_records_on_device(BuildInput{offsets.as<uint64_t>(), nodes.as<uint32_t>(), n, total, false, min_node, max_node}, o, s);
    o.peak_scratch += sc.peak;
    return GBWT_HIP_OK;
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_merge(const gbwt_hip_index *a, const gbwt_hip_index *b, const gbwt_hip_merge_options *opts, uint32_t flags, gbwt_hip_index **out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = nullptr;
    if (!a || !b) return fail(GBWT_HIP_BAD_ARGUMENT, "null index");
    gbwt_hip_status st = check_open_flags(flags);
    if (st != GBWT_HIP_OK) return st;
    uint32_t algorithm = GBWT_HIP_MERGE_AUTO;
    if (opts) {
        if (opts->algorithm > GBWT_HIP_MERGE_INSERT) return fail(GBWT_HIP_BAD_ARGUMENT, "options: algorithm is one of GBWT_HIP_MERGE_AUTO | _REBUILD | _INSERT");
        if (opts->reserved32 != 0 || opts->reserved[0] != 0 || opts->reserved[1] != 0) return fail(GBWT_HIP_BAD_ARGUMENT, "options: reserved must be 0");
        algorithm = opts->algorithm;
    }
    const HostIndex &ha = a->host, &hb = b->host;
    if (a->device != b->device) return fail(GBWT_HIP_BAD_ARGUMENT, "the two indexes are on different devices (" + std::to_string(a->device) + " and " + std::to_string(b->device) + ")");
    if (ha.bidirectional != hb.bidirectional) return fail(GBWT_HIP_BAD_ARGUMENT, "one index is bidirectional and the other is not");
    if (ha.is_gbz != hb.is_gbz) return fail(GBWT_HIP_BAD_ARGUMENT, "one index is a GBZ and the other a bare GBWT");
    if (algorithm == GBWT_HIP_MERGE_INSERT && !ha.bidirectional) return fail(GBWT_HIP_BAD_ARGUMENT, "options: GBWT_HIP_MERGE_INSERT needs bidirectional indexes");
    // AUTO: the rebuild, which was measured faster on both shapes of tools/merge_bench.py, where it can run -- it extracts
    // the sequences --, else the insertion, which reads only what every handle keeps
    if (algorithm == GBWT_HIP_MERGE_AUTO) {
        const bool extractable = (a->caps & GBWT_HIP_OPEN_EXTRACT) && (b->caps & GBWT_HIP_OPEN_EXTRACT);
        algorithm = (extractable || !ha.bidirectional) ? GBWT_HIP_MERGE_REBUILD : GBWT_HIP_MERGE_INSERT;
    }

    // the widths of the construction over the merged set
    const MergeInput ia = input_of(a), ib = input_of(b);
    const uint64_t sequences = ia.sequences + ib.sequences, visits = ia.visits + ib.visits;
    st = check_build_sizes(sequences, visits, 0);
    if (st != GBWT_HIP_OK) return st;
    BuildOutput o;
    o.sequences = sequences; o.visits = visits; o.alphabet_offset = 0; o.alphabet_size = 1;
    if (visits) {
        o.alphabet_offset = ~uint64_t(0);
        for (const MergeInput *x : {&ia, &ib})
            if (x->visits) { o.alphabet_offset = std::min(o.alphabet_offset, x->alphabet_offset); o.alphabet_size = std::max(o.alphabet_size, x->alphabet_size); }
        st = check_build_range(o.alphabet_offset + 1, o.alphabet_size - 1);
        if (st != GBWT_HIP_OK) return st;
    }
    o.records = o.alphabet_size - o.alphabet_offset;

    // metadata, tags, graph: on the host, from what the handles hold
    const auto t_meta = Clock::now();
    HostIndex meta;
    MergeRefusal bad = merge_metadata(ha, hb, meta);
    if (bad) return refusal_status(bad, "merge: ");
    if (ha.is_gbz) {
        bad = merge_graph(ha, hb, o.alphabet_offset, o.alphabet_size, meta);
        if (bad) return refusal_status(bad, "merge: ");
    }
    meta.tags = merge_tags(ha.tags, hb.tags);
    meta.gbz_tags = merge_tags(ha.gbz_tags, hb.gbz_tags);
    const double metadata_ms = ms_since(t_meta);

    st = require_device();
    if (st != GBWT_HIP_OK) return st;
    const int device = a->device;
    try {
        HIP_CHECK(hipSetDevice(device));
        Stream stream;
        MergeWalk walk;
        if (visits == 0) build_without_visits(sequences, o);
        else if (algorithm == GBWT_HIP_MERGE_REBUILD) {
            st = rebuild(a, b, o.alphabet_offset + 1, o.alphabet_size - 1, o, stream.s);
            if (st != GBWT_HIP_OK) return st;
        } else merge_records_on_device(ia, ib, o, walk, stream.s);

        const auto t_open = Clock::now();
        std::unique_ptr<gbwt_hip_index> ix = handle_from_build(o, ha.bidirectional, device, flags);
        adopt_metadata(ix->host, std::move(meta));

        gbwt_hip_merge_info m{};
        fill_build_counters(m, o);
        m.walked_sequences = walk.walked_sequences; m.walked_steps = walk.walked_steps;
        m.algorithm_used = algorithm; m.walked_input = walk.walked_input; m.merged = 1;
        m.walk_ms = walk.walk_ms; m.decode_ms = walk.decode_ms; m.interleave_ms = walk.interleave_ms;
        m.metadata_ms = metadata_ms;
        st = open_host_index(std::move(ix), out, t_open);
        if (st != GBWT_HIP_OK) return st;
        m.open_ms = ms_since(t_open);
        (*out)->merge_info = m;
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e, "the merge");
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_merge_info(const gbwt_hip_index *ix, gbwt_hip_merge_info *out) {
    GBWT_HIP_GUARD_BEGIN
    return last_info(ix, out, &gbwt_hip_index::merge_info);
    GBWT_HIP_GUARD_END
}

}  // extern "C"
