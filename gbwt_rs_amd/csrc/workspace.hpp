// workspace.hpp -- gbwt_hip_workspace, the workspace of the C ABI: one struct of state per request family, each with its buffers, its events
// (made by the family's first request) and the memo of the request its results answer.  A family's translation unit touches its own struct
// and `scratch`; what it reads of another family is spelled ws-><that family>.
#pragma once

#include <mutex>
#include <string>
#include <vector>

#include "capi_status.hpp"
#include "device_buffer.hpp"
#include "handle.hpp"
#include "hip_raii.hpp"
#include "knobs.hpp"
#include "request_key.hpp"

namespace gbwt_hip {

// The pinned staging buffers and streams of a workspace's device-to-host copies (capi_extract.hip: copy_to_host), made on first use.
struct HostCopier {
    static constexpr size_t CHUNK = size_t(16) << 20;
    struct Lane { void *pinned[2] = {nullptr, nullptr}; hipEvent_t landed[2] = {nullptr, nullptr}; hipStream_t stream = nullptr; };
    std::vector<Lane> lanes;
    std::mutex busy;
    HostCopier() = default;
    HostCopier(const HostCopier &) = delete;
    HostCopier &operator=(const HostCopier &) = delete;
    ~HostCopier();
    bool ensure(int device, unsigned threads);
};

// What a suffix array request needs beside its scratch (suffix_array.hip): events -- [0] .. [7] the text (the caller's), [1] .. [2] the pack, [2] .. [3]
// the ranking, [3] .. [4] the output, [5] .. [6] one round -- and the pinned words the size of the active set and the runs are read through
struct SaContext {
    EventSet<8> ev{OnFirstUse{}};
    PinnedWords words;
    void ensure() { ev.ensure(); words.ensure(); }
};

// Extraction (capi_extract.hip; comm.hip reads the rows).  The rows of the last request -- ids, offsets, nodes -- are what the lines, bases,
// tags and positions are made from: those families read seq_ids, ev, timed and pinned_words here.  ev[3] .. ev[2]: everything the
// extraction put on the stream, ev[0] .. ev[1]: its walk; made with the workspace.  memo: the ids of the rows (whole rows only).
struct ExtractState {
    DeviceBuffer seq_ids, lengths, offsets, head, pool, next, counters, nodes;
    DeviceBuffer order_keys, order_rows, order_counts, order_level, order_temp;   // walker order of a segmented extraction
    uint64_t device_bytes() const { return bytes_of({&seq_ids, &lengths, &offsets, &head, &pool, &next, &counters, &nodes, &order_keys, &order_rows, &order_counts, &order_level, &order_temp}); }
    uint64_t rows_bytes() const { return nodes.bytes; }
    uint64_t rows_chunks() const { return nodes.chunks.size(); }
    EventSet<4> ev{OnFirstUse{}};
    PinnedWords pinned_words;              // the total and extremes of a request whose rows are sized after its launch
    bool timed = false;
    uint64_t last_n = 0, last_total = 0;   // shape of the last device-resident extraction
    RequestKey memo;
};

// Navigation and search (capi_query.hip): staging of the queries and their results.  ev: around the kernel(s) of the last call -- an
// edges / links request (capi_topology.hip) reports its time through them as well.  memo: the states and direction of a follow request.
struct QueryState {
    DeviceBuffer in_a, in_b, out_a, out_valid, follow_off;   // out_a also takes the per-row checksums of an extraction (capi_extract.hip: path_sums)
    uint64_t device_bytes() const { return bytes_of({&in_a, &in_b, &out_a, &out_valid, &follow_off}); }
    EventSet<2> ev{OnFirstUse{}};
    bool timed = false;
    uint64_t follow_total = 0;
    RequestKey memo;
};

// GFA path lines (capi_lines.hip; comm.hip gathers them): line lengths and starts, the text (text2: the second text buffer of a pipelined
// whole-file write).  ev: around the formatting of the last request (behind its walk).  memo: path ids, line mode and text slot.
struct LinesState {
    DeviceBuffer b, c, text, text2, valid;
    uint64_t device_bytes() const { return bytes_of({&b, &c, &text, &text2, &valid}); }
    uint64_t text_bytes() const { return text.bytes + text2.bytes; }
    EventSet<2> ev{OnFirstUse{}};
    bool timed = false;
    uint64_t total = 0;
    RequestKey memo;
    uint64_t n = 0;                        // paths and text slot of the request the memo holds (what gbwt_hip_gather_lines gathers)
    int slot = 0;
};

// Bases of paths (sequences.hip, capi_sequences.hip): text and row offsets of the last gbwt_hip_path_sequences* request (text2: the second text buffer of a
// pipelined whole-file write).  ev[0] .. ev[1]: its sizing, ev[1] .. ev[2]: its bases kernel.  memo: path ids, reverse, endmarker, slot.
struct BasesState {
    DeviceBuffer text, text2, offsets;
    uint64_t device_bytes() const { return bytes_of({&text, &text2, &offsets}); }
    uint64_t text_bytes() const { return text.bytes + text2.bytes; }
    EventSet<3> ev{OnFirstUse{}};
    bool timed = false;
    uint64_t total = 0;
    RequestKey memo;
};

// Tags of a suffix array (tags.hip, capi_tags.hip).  The PLAN of the last list of path ids (plan_key): for every position of the text's walk -- the nodes of
// the rows and one endmarker position behind each -- its node (node, u32) and its text offset (off, u64, one more entry = the text length),
// and the sampled top level (top: the position that holds text offset h << TAG_SHIFT; u32, u64 from 2^32 positions).  rows: the text offset
// of every row (+ the text length) on the host.  state: run count, last tags and the out-of-range flag of a request; sa* / out*: the
// staging of the host and file forms.  Times of the last request: the plan's are kept with the plan.
struct TagsState {
    DeviceBuffer node, off, top, state, sa, sa2, out, out2;
    uint64_t device_bytes() const { return bytes_of({&node, &off, &top, &state, &sa, &sa2, &out, &out2}); }
    EventSet<2> ev{OnFirstUse{}};
    bool timed = false, wide = false;
    RequestKey plan_key;
    std::vector<uint64_t> rows;
    uint64_t positions = 0, text_len = 0;
    float walk_ms = 0, plan_ms = 0, gather_ms = 0;
};

// Suffix array and BWT of the text of paths (suffix_array.hip, capi_suffix_array.hip).  The results of the last request: sa holds 16 bytes of
// lead -- the entry `total` of a .sa file in its second word -- and then the u64 suffix array; bwt 16 bytes of lead -- the byte T[total - 1] of
// a .bwt file in its last -- and then the BWT: a file is one stretch of either buffer.  The text is the bases family's (ws->bases.text).
// The scratch of the ranking is the builder's own and gone when a request returns.  ev: see SaContext.  memo: path ids and endmarker.
struct SuffixState {
    DeviceBuffer sa, bwt;
    uint64_t device_bytes() const { return bytes_of({&sa, &bwt}); }
    SaContext ctx;
    bool built = false;
    uint64_t total = 0;
    gbwt_hip_suffix_array_info info{};
    RequestKey memo;
};

// Reference positions (refpos.hip, capi_refpos.hip).  Scratch of the last request, per position (node of its rows): off (u64 bases in front
// of it), mark (u64: its label length, then whether it is kept), jump (two u32 jump arrays, then its u64 slot); rows: the sequence ids,
// path ids and segment counts of the rows; flags: a word per pointer-doubling round, one for the walk.  Results: paths[n],
// positions[total].  ev[0] .. ev[1]: the selection, ev[1] .. ev[2]: the walk that writes the positions.  memo: path ids and interval.
struct RefposState {
    DeviceBuffer off, mark, jump, rows, flags, paths, positions;
    uint64_t device_bytes() const { return bytes_of({&off, &mark, &jump, &rows, &flags, &paths, &positions}); }
    EventSet<3> ev{OnFirstUse{}};
    bool timed = false;
    uint64_t total = 0;
    uint32_t rounds = 0, launches = 0;
    float walk_ms = 0, select_ms = 0, offsets_ms = 0;
    RequestKey memo;
};

// Edges and links of the graph API (topology.hip, capi_topology.hip).  Rows of the last request: its queries (ids u64, orient u8; seg: the
// segment ids of a links request), counts, offsets, edges, the query of every edge (rows, links only), valid bytes and the list of long
// rows (big); for links the cuts, the link offsets and the links.  memo: ids, orientations, links / predecessors and n.
struct EdgesState {
    DeviceBuffer ids, orient, seg, counts, off, edges, rows, valid, big, cut, loff, links;
    uint64_t device_bytes() const { return bytes_of({&ids, &orient, &seg, &counts, &off, &edges, &rows, &valid, &big, &cut, &loff, &links}); }
    uint64_t n = 0, total = 0;
    RequestKey memo;
};

// Graph lines (capi_topology.hip): the items of the S-lines (node or segment ids) and their line offsets, the edge rows of all (node |
// segment, orientation) pairs with the query of every edge and the offsets of their L-lines -- kept from the first request (sized), so
// that a later one only formats -- and the text.  ev[0] .. [1] sizing, [1] .. [2] S-lines, [2] .. [3] L-lines.
struct GraphTextState {
    DeviceBuffer items, soff, edges, rows, loff, text;
    uint64_t device_bytes() const { return bytes_of({&items, &soff, &edges, &rows, &loff, &text}); }
    uint64_t text_bytes() const { return text.bytes; }
    EventSet<4> ev{OnFirstUse{}};
    bool sized = false, text_valid = false, timed = false, translated = false, sized_now = false;   // sized_now: the last request sized
    uint64_t item_count = 0, edge_count = 0, sbytes = 0, lbytes = 0, links = 0;
    std::string header;
};

// Locate (locate.hip, capi_locate.hip).  The rows of the last request -- off / ids / valid, for a unique request uoff and the compacted
// ids -- live in buffers of their own: an edges / links request leaves them alone.  states: the states of a request given on the host;
// counts, keys, sorted, flag, rank, temp: scratch; words: the flag word and the step counter; pos / pos_ids / pos_valid: a
// positions request.  ev[0] .. ev[1]: the locate kernel, ev[1] .. ev[2]: sort and compaction of a unique request.  memo: states, unique, n.
struct LocateState {
    DeviceBuffer states, counts, off, ids, valid, keys, sorted, flag, rank, uoff, temp, words, pos, pos_ids, pos_valid;
    uint64_t device_bytes() const { return bytes_of({&states, &counts, &off, &ids, &valid, &keys, &sorted, &flag, &rank, &uoff, &temp, &words, &pos, &pos_ids, &pos_valid}); }
    EventSet<3> ev{OnFirstUse{}};
    bool timed = false, compacted = false;   // compacted: uoff holds the offsets of the rows (a unique request with ids)
    uint64_t n = 0, total = 0, steps = 0;
    float walk_ms = 0, sort_ms = 0;
    RequestKey memo;
};

// Scratch of any family: the temporary storage of scans and sorts, and the per-row words and chunk plan of a pass over a batch of rows
// (capi_lines.hip, capi_sequences.hip, capi_tags.hip).  Nothing in it survives a request: a family sizes and fills it before it reads it, and assumes
// nothing about it once any other entry point has run on the workspace.
struct ScratchState {
    DeviceBuffer scan_temp, a, chunk_first, chunks, plan;
    uint64_t device_bytes() const { return bytes_of({&scan_temp, &a, &chunk_first, &chunks, &plan}); }
};

}  // namespace gbwt_hip

struct gbwt_hip_workspace {
    const gbwt_hip_index *index = nullptr;
    ExtractKnobs knobs;              // (with the walk mode, paths per wave and small-record size of gbwt_hip_workspace_tune)
    gbwt_hip::ExtractState extract;
    gbwt_hip::QueryState query;
    gbwt_hip::LinesState lines;
    gbwt_hip::BasesState bases;
    gbwt_hip::TagsState tags;
    gbwt_hip::SuffixState suffix;
    gbwt_hip::RefposState refpos;
    gbwt_hip::EdgesState edges;
    gbwt_hip::GraphTextState graph_text;
    gbwt_hip::LocateState locate;
    gbwt_hip::ScratchState scratch;
    gbwt_hip::HostCopier copier;     // pinned staging of the large device-to-host copies
    gbwt_hip::Stream stream{gbwt_hip::OnFirstUse{}};   // made by gbwt_hip_workspace_create, on the handle's device; the last member: it goes first, before the buffers its work used
    uint64_t device_bytes() const {
        return extract.device_bytes() + query.device_bytes() + lines.device_bytes() + bases.device_bytes() + tags.device_bytes() + suffix.device_bytes() + refpos.device_bytes() + edges.device_bytes() +
               graph_text.device_bytes() + locate.device_bytes() + scratch.device_bytes();
    }
    uint64_t text_bytes() const { return lines.text_bytes() + bases.text_bytes() + graph_text.text_bytes(); }
};

namespace gbwt_hip {

// Device -> pageable host memory over the workspace's copy threads (GBWT_HIP_COPY_THREADS, default 8), each with two pinned staging
// buffers and a stream of its own (capi_extract.hip)
void copy_to_host(gbwt_hip_workspace *ws, void *dst, const void *src, size_t bytes, size_t piece = HostCopier::CHUNK);

}  // namespace gbwt_hip
