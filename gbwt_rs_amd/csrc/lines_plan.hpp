// lines_plan.hpp -- every decision of a GFA lines request (capi_lines.hip) as arithmetic over numbers the host has: plain C++, no HIP and
// no workspace (tests/cpp/lines_plan.cpp runs it without a GPU).  How many chunks a batch of rows may have and when that is refused, where
// the scratch arrays of the sizing pass lie in the workspace's buffers, which of the three sizing passes a handle takes, and -- for the
// whole-file writer -- the passes over the paths, the widest token and where a byte-bounded batch ends.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gbwt_hip {

// Lines are formatted in chunks of LINE_CHUNK path positions, so that the work is as parallel for ninety haplotypes of two
// million nodes as it is for fifty thousand short walks (one workgroup per LINE had 0.6 G nodes/s on the former, 50 on the
// latter).  Every row has at least one chunk (an empty path still has a header and a trailer).
constexpr uint32_t LINE_CHUNK = 4096;   // (= GFA_LINE_CHUNK, kernels.hpp: the line cache is filled per chunk of this size at open)

// The number of chunks of a request is known on the device only; the host launches and scans over this upper bound: a row of len
// positions has at most len / LINE_CHUNK + 1 chunks.  The kernels index chunks with 32 bits: a larger bound is refused.
constexpr uint64_t CHUNKS_MAX = 0x7FFFFFFFull;
constexpr const char *LINES_TOO_MANY_CHUNKS = "too many line chunks in one batch: format fewer paths per call";
constexpr const char *TOKENS_TOO_MANY_CHUNKS = "too many chunks in one batch: ask for fewer paths per call";
struct ChunksCap { uint64_t chunks; bool refused; };
inline ChunksCap chunks_cap(uint64_t total, uint64_t n) {
    const uint64_t chunks = total / LINE_CHUNK + n;
    return ChunksCap{chunks, chunks > CHUNKS_MAX};
}

// ---- scratch layouts ----------------------------------------------------------------------------------------------------------------
// Where the arrays of a request lie in ScratchState::a, ::chunk_first and ::chunks (workspace.hpp): offsets in 64-bit words from the start
// of the buffer, and the bytes to reserve for it.  The request gets every pointer from the layout (scratch_at), so the size and the
// places cannot drift apart.  chunk_path is an array of 32-bit words behind the 64-bit ones.
template <class T>
inline T *scratch_at(void *buffer, uint64_t word) { return reinterpret_cast<T *>(static_cast<uint64_t *>(buffer) + word); }

// a lines request: per row the length of its line and its W-line end coordinate; per chunk text bytes, label lengths and the flag of a
// position that fits no segment, and the scans of the three ([chunks_cap + 1] each)
struct LinesLayout {
    uint64_t line_len, line_end, a_bytes;                                                    // scratch.a
    uint64_t chunk_first, chunk_counts, chunk_first_bytes;                                   // scratch.chunk_first
    uint64_t chunk_text, chunk_seq, chunk_bad, text_before, seq_before, bad_before, chunk_path, chunks_bytes;   // scratch.chunks
};
inline LinesLayout lines_layout(uint64_t n, uint64_t cap) {
    LinesLayout l;
    l.line_len = 0; l.line_end = n; l.a_bytes = 2 * n * sizeof(uint64_t);
    l.chunk_first = 0; l.chunk_counts = n + 1; l.chunk_first_bytes = 2 * (n + 1) * sizeof(uint64_t);
    l.chunk_text = 0; l.chunk_seq = cap; l.chunk_bad = 2 * cap;
    l.text_before = 3 * cap; l.seq_before = l.text_before + (cap + 1); l.bad_before = l.seq_before + (cap + 1);
    l.chunk_path = l.bad_before + (cap + 1);
    l.chunks_bytes = l.chunk_path * sizeof(uint64_t) + (cap + 1) * sizeof(uint32_t);
    return l;
}

// a segment tokens request (gbwt_hip_segment_paths): per row its tokens and where they start; per chunk tokens and the flag, and their scans
struct TokensLayout {
    uint64_t row_tokens, row_start, a_bytes;
    uint64_t chunk_first, chunk_counts, chunk_first_bytes;
    uint64_t chunk_tokens, chunk_bad, tokens_before, bad_before, chunk_path, chunks_bytes;
};
inline TokensLayout tokens_layout(uint64_t n, uint64_t cap) {
    TokensLayout l;
    l.row_tokens = 0; l.row_start = n + 1; l.a_bytes = 2 * (n + 1) * sizeof(uint64_t);
    l.chunk_first = 0; l.chunk_counts = n + 1; l.chunk_first_bytes = 2 * (n + 1) * sizeof(uint64_t);
    l.chunk_tokens = 0; l.chunk_bad = cap;
    l.tokens_before = 2 * cap; l.bad_before = l.tokens_before + (cap + 1);
    l.chunk_path = l.bad_before + (cap + 1);
    l.chunks_bytes = l.chunk_path * sizeof(uint64_t) + (cap + 1) * sizeof(uint32_t);
    return l;
}

// ---- how the lines of a request are sized -------------------------------------------------------------------------------------------
// Cached: from the line cache of the index (lc_state == 1: filled at open), no node id is read before the formatter reads it.
// Plain: a wave per chunk sums token bytes and label lengths.  Translated: the same over segment tokens, with a flag for every path that
// is not a concatenation of whole segments (the host replays those).  A translation graph has no line cache.
enum class LineSizing { Cached, Plain, Translated };
inline LineSizing line_sizing(bool translated, int lc_state) {
    if (translated) return LineSizing::Translated;
    return lc_state == 1 ? LineSizing::Cached : LineSizing::Plain;
}

// ---- the whole-file writer (gbwt_hip_write_gfa_mode) --------------------------------------------------------------------------------
// write_gfa_impl's match on the path mode (src/bin/gbunzip.rs:212-222), ascending path id (-t 1 order):
//   default (0): paths of the generic sample as P-lines, then the others as W-lines (write_paths / write_walks, 343-417)
//   pan-sn  (1): every path as a P-line with its PanSN name (write_pan_sn, 371-393)
//   ref-only (2): the P-lines of the default mode only
// have_ref: the metadata has sample names and the generic sample among them.
struct LinePass { int line_mode; int which; };     // which: 0 = paths of the generic sample, 1 = the others, 2 = all
inline bool operator==(const LinePass &a, const LinePass &b) { return a.line_mode == b.line_mode && a.which == b.which; }
inline std::vector<LinePass> gfa_passes(int path_mode, bool have_ref) {
    std::vector<LinePass> passes;
    if (path_mode == 1) passes.push_back(LinePass{2, 2});
    else {
        if (have_ref) passes.push_back(LinePass{0, 0});
        if (path_mode == 0) passes.push_back(LinePass{1, 1});
    }
    return passes;
}

// a path of `len` nodes prints at most len tokens of (digits of the largest node id, or the longest segment name) + 2 bytes
inline uint64_t token_width_bound(uint64_t largest_node_id, bool translated, uint64_t longest_segment_name) {
    if (translated) return 2 + longest_segment_name;
    uint64_t digits = 1;
    for (uint64_t v = largest_node_id; v >= 10; v /= 10) digits++;
    return 2 + digits;
}

// The paths ids[b0 ...] that go into the next batch: as many as fit `budget` bytes of text by the estimate 128 + token * (nodes of the
// path), the first one always (a path larger than the budget goes alone).  seq_len: the host's copy of the sequence lengths (the forward
// sequence of path p is sequence 2p); a sequence beyond it estimates 0, and without any the batches are cut by count, `fallback` paths each.
inline uint64_t next_batch(const uint64_t *ids, uint64_t count, uint64_t b0, const uint32_t *seq_len, uint64_t n_seq_len, uint64_t token, uint64_t budget, uint64_t fallback) {
    uint64_t nb = 0, bytes = 0;
    while (b0 + nb < count) {
        const uint64_t seq = 2 * ids[b0 + nb];
        const uint64_t est = seq < n_seq_len ? 128 + token * seq_len[seq] : 0;
        if (nb != 0 && (n_seq_len == 0 ? nb >= fallback : bytes + est > budget)) break;
        bytes += est; nb++;
    }
    return nb;
}

}  // namespace gbwt_hip
