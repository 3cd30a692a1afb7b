// fm_object.hpp -- the FM-index object of the C ABI as its translation units see it (capi_fm.hip: the build and count / locate / graph
// positions; capi_fm_seeds.hip: the seeds of reads; capi_fm_chains.hip: their chains; capi_fm_align.hip: the kept text and the alignments
// of the chains), and the checks of a request that they make before any device work.
#pragma once

#include <string>
#include <vector>

#include "capi_internal.hpp"
#include "fm_layout.hpp"

// The rows of the last seeds request of an object, and what it was
struct gbwt_hip_fm_seed_state {
    gbwt_hip::DeviceBuffer q_offsets, q_bytes;                 // reads given on the host
    gbwt_hip::DeviceBuffer read_offsets, seeds, hit_offsets, positions, tags;
    gbwt_hip::EventSet<5> ev{gbwt_hip::OnFirstUse{}};
    gbwt_hip::RequestKey memo;
    uint64_t m = 0, total_seeds = 0, total_hits = 0;
    bool with_hits = false, with_tags = false;
    gbwt_hip_fm_seed_info info{};
};

// The rows of the last chains request of an object, and what it was
struct gbwt_hip_fm_chain_state {
    gbwt_hip::DeviceBuffer read_offsets, chains, match_offsets, matches;      // (reads given on the host lie in the seeds state)
    // (the list stands under the buffers.  An FM-index is no part of gbwt_hip_memory_usage, which sums a handle and its
    // workspaces, so nothing reports this sum yet; gbwt_hip_fm_last_chain_info reports the path offsets, which the object keeps for good)
    uint64_t device_bytes() const { return gbwt_hip::bytes_of({&read_offsets, &chains, &match_offsets, &matches}); }
    gbwt_hip::EventSet<6> ev{gbwt_hip::OnFirstUse{}};
    gbwt_hip::RequestKey memo;
    uint64_t m = 0, total_chains = 0, total_matches = 0;
    gbwt_hip_fm_chain_info info{};
};

// The rows of the last alignments request of an object, and what it was
struct gbwt_hip_fm_align_state {
    gbwt_hip::DeviceBuffer q_offsets, q_bytes;                 // reads given on the host: a copy of its own, whatever the seeds state holds by now
    gbwt_hip::DeviceBuffer read_offsets, alignments, cigar_offsets, cigars;
    uint64_t device_bytes() const { return gbwt_hip::bytes_of({&q_offsets, &q_bytes, &read_offsets, &alignments, &cigar_offsets, &cigars}); }
    gbwt_hip::EventSet<4> ev{gbwt_hip::OnFirstUse{}};
    gbwt_hip::RequestKey memo;
    uint64_t m = 0, total_alignments = 0, total_cigars = 0;
    gbwt_hip_fm_align_info info{};
};

// One FM-index: what fm_layout.hpp describes in HBM, the rows of its last request, and -- for an index of paths -- what the graph-position
// call needs to turn text positions into tags.  One host thread at a time.
struct gbwt_hip_fm_index {
    int device = 0;
    // the index
    gbwt_hip::DeviceBuffer lines, counts, tables, sa;
    uint64_t index_bytes() const { return gbwt_hip::bytes_of({&lines, &counts, &tables, &sa}); }
    gbwt_hip::FmLayout layout;
    uint64_t n = 0;
    bool count_only = false;
    // the paths behind a path-level index
    const gbwt_hip_index *index = nullptr;
    std::vector<uint64_t> path_ids;
    int endmarker = 0;
    gbwt_hip::DeviceBuffer path_offsets;                  // [path_ids.size() + 1] text offsets of the paths, each with its endmarker: the segments of the chains
    // the text, where the caller gave it to the object (gbwt_hip_fm_set_text, gbwt_hip_fm_keep_path_text): what the alignments read
    gbwt_hip::DeviceBuffer text;
    bool has_text = false;
    // the last request: patterns given on the host, ranges and occurrence counts, row offsets, positions, the row of every position, tags;
    // sorted_* / flag / rank / uoff / kept: a unique request; words: [0] flags, [1] backward steps
    gbwt_hip::DeviceBuffer q_offsets, q_bytes, ranges, occ, roff, positions, rows, tags, tmp_values, tmp_rows, sorted_values, sorted_rows, flag, rank, uoff, kept, temp, words;
    gbwt_hip::EventSet<3> ev{gbwt_hip::OnFirstUse{}};
    gbwt_hip::RequestKey memo;
    bool unique_rows = false;         // uoff / kept answer the last request
    uint64_t last_m = 0, last_total = 0;
    gbwt_hip_fm_index_info info{};
    gbwt_hip_fm_seed_state seed;      // the last seeds request: rows of its own, beside those of the queries above
    gbwt_hip_fm_chain_state chain;    // the last chains request: rows of its own, beside the seeds rows it was made from
    gbwt_hip_fm_align_state align;    // the last alignments request: rows of its own, beside the chains rows it was made from
    gbwt_hip::Stream stream{gbwt_hip::OnFirstUse{}};      // the last member: it goes first, before the buffers its work used
};

namespace gbwt_hip {

enum FmKind { FM_COUNT = 0, FM_LOCATE = 1, FM_GRAPH = 2 };

// The checks of a query that answer before any device work: first the outputs and the patterns, then the object
inline gbwt_hip_status fm_check_patterns(const uint64_t *offsets, const void *bytes, uint64_t m, bool on_host) {
    if (!offsets) return fail(GBWT_HIP_BAD_ARGUMENT, "null pattern offsets (m + 1 of them, also for m == 0)");
    if (m >= 0x7FFFFFFFull) return fail(GBWT_HIP_BAD_ARGUMENT, "too many patterns in one request (at most 2^31 - 2)");
    if (!on_host) return GBWT_HIP_OK;
    for (uint64_t k = 0; k < m; k++)
        if (offsets[k + 1] < offsets[k]) return fail(GBWT_HIP_BAD_ARGUMENT, "pattern offsets do not ascend at pattern " + std::to_string(k));
    if (offsets[m] != 0 && !bytes) return fail(GBWT_HIP_BAD_ARGUMENT, "null pattern bytes");
    return GBWT_HIP_OK;
}

inline gbwt_hip_status fm_check_object(const gbwt_hip_fm_index *fm, FmKind kind, const gbwt_hip_index *ix, const gbwt_hip_workspace *ws, int unique) {
    if (!fm) return fail(GBWT_HIP_BAD_ARGUMENT, "null FM-index");
    if (unique != 0 && unique != 1) return fail(GBWT_HIP_BAD_ARGUMENT, "unique must be 0 or 1");
    if (kind != FM_COUNT && fm->count_only) return fail(GBWT_HIP_UNSUPPORTED, "a count-only FM-index holds no suffix array: nothing to locate with");
    if (kind == FM_GRAPH) {
        if (!fm->index) return fail(GBWT_HIP_BAD_ARGUMENT, "graph positions need an FM-index made by gbwt_hip_path_fm_index, not one of a plain text");
        if (!ix || ix != fm->index) return fail(GBWT_HIP_BAD_ARGUMENT, "the FM-index was made from another index handle");
        if (!ws || ws->index != ix) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    }
    return GBWT_HIP_OK;
}

// The seed options as every request that takes them checks them, behind the reads and in front of the object
inline gbwt_hip_status fm_check_seed_options(const gbwt_hip_fm_seed_options &opts) {
    if (opts.strands < 1 || opts.strands > 3) return fail(GBWT_HIP_BAD_ARGUMENT, "strands: 1 (forward), 2 (reverse) or 3 (both)");
    if (opts.flags != 0 || opts.reserved != 0) return fail(GBWT_HIP_BAD_ARGUMENT, "flags and reserved of the seed options must be 0");
    return GBWT_HIP_OK;
}

// The rows of a seeds request into the object's seeds state (capi_fm_seeds.hip), for the requests that start with one.  Exactly one of
// h_offsets / d_offsets; bytes: the read bytes behind d_bytes (the host form: offsets[m]).  The request has passed its checks.
gbwt_hip_status fm_seeds_compute(gbwt_hip_fm_index *fm, const uint64_t *h_offsets, const void *h_bytes, const uint64_t *d_offsets, const uint8_t *d_bytes, uint64_t m, uint64_t bytes,
                                 const gbwt_hip_fm_seed_options &opts, bool graph, const gbwt_hip_index *ix, gbwt_hip_workspace *ws);

// The checks of a chains request in front of the object (capi_fm_chains.hip): the reads, the seed options, the chain options.  Null
// options become the defaults
gbwt_hip_status fm_check_chain_request(const uint64_t *offsets, const void *bytes, uint64_t m, bool on_host, const gbwt_hip_fm_seed_options *&seed_opts,
                                       const gbwt_hip_fm_chain_options *&chain_opts);
// The rows of a chains request into the object's chains state, through its memo (capi_fm_chains.hip), for the requests that start with one
gbwt_hip_status fm_chains_compute(gbwt_hip_fm_index *fm, const uint64_t *h_offsets, const void *h_bytes, const uint64_t *d_offsets, const uint8_t *d_bytes, uint64_t m, uint64_t bytes,
                                  const gbwt_hip_fm_seed_options &seed_opts, const gbwt_hip_fm_chain_options &chain_opts);

}  // namespace gbwt_hip
