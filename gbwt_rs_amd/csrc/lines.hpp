// lines.hpp -- launch wrappers of lines.hip: the P- and W-lines of a batch of extracted rows, and GBZ::segment_path as data.  The tables the
// kernels read are handed over as the small structs below; the rows of a request and their chunks as ChunkedRows.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "lines_plan.hpp"

namespace gbwt_hip {

static_assert(LINE_CHUNK == GFA_LINE_CHUNK, "the line cache is filled at open per chunk of the size the formatter works in");

// The headers of one line mode as the kernels see them (gbwt_hip_index::line_prefix): everything in front of the node tokens, per path of
// the metadata.  W-lines (fragment != null) end in "<fragment>\t<fragment + summed label lengths>\t" (path_to_w_line,
// src/bin/gbunzip.rs:532-540): the table holds the line up to and including "<fragment>\t", the end coordinate and its tab are
// appended where the line is formatted.
struct LineHeaders {
    const uint8_t *prefix;
    const uint64_t *prefix_off;    // [paths + 1]
    const uint32_t *fragment;      // [paths], or null: no end coordinate (P-lines)
};

// The line cache of the index as the kernels see it (gbwt_hip_index::lc_*): per path its first chunk, per chunk the W-line token bytes of
// the path in front of the chunk, per path {its W-line token bytes, its summed label lengths}.  A W-line token is '>' + digits, a P-line
// token digits + '+' and a ',' in front of all but the first: the P-line text in front of chunk k is the W-line text + cache_p_extra(k).
struct LineCache { const uint64_t *chunk_first; uint64_t *text; uint64_t *path; };

// What the workgroup of a chunk starts from, put together once per request by one thread per chunk: where its node ids and its text begin, how
// many positions it has, whether it opens / closes its line.  The workgroups used to find all that themselves -- four levels of dependent
// loads and the decimal length of the W-line's end coordinate in every one of their 256 threads -- before they asked for their first node id.
struct __attribute__((aligned(16))) ChunkPlan {
    uint64_t ids_at;        // index of the chunk's first position in the rows
    uint64_t text_at;       // byte of the text where its first token begins
    uint32_t count, row;    // positions; the request's row (= line) it belongs to
    uint32_t flags;         // 1: first chunk of its line (writes the header), 2: last (writes the trailer)
    uint32_t header_len;
};
static_assert(sizeof(ChunkPlan) == 32, "two 16-byte loads");

// The translation tables as the kernels see them.
struct SegmentTables {
    const uint32_t *seg_of;
    const uint32_t *seg_start;
    const uint64_t *name_off;
    const uint8_t *names;
    const uint64_t *seq_len;
    const uint8_t *node_real;
    uint64_t mapping_len;
};

// The rows of a request (CSR: offsets[n + 1], nodes) cut into chunks of LINE_CHUNK positions: chunk c belongs to the row with
// chunk_first[row] <= c < chunk_first[row + 1], which is chunk_path[c].  The number of chunks is chunk_first[n], known on the device
// only: launches and scans run over the host's bound chunks_cap (lines_plan.hpp), and the chunks past the end count nothing.
struct ChunkedRows {
    const uint64_t *offsets;
    const uint32_t *nodes;
    uint64_t n;
    const uint64_t *chunk_first;   // [n + 1]
    const uint32_t *chunk_path;    // [chunks_cap]
    uint64_t chunks_cap;
};

// The chunk plan of a batch of rows, for the lines and for other passes over rows (the bases of sequences.hip): first chunk of every row
// (d_chunk_first[n + 1], d_chunk_counts[n] scratch) and the row of every chunk (d_chunk_path[chunks_cap]).
void launch_chunk_plan(const uint64_t *d_offsets, uint64_t n, uint64_t chunks_cap, uint64_t *d_chunk_counts, uint64_t *d_chunk_first, uint32_t *d_chunk_path, void *d_temp,
                       size_t temp_bytes, hipStream_t s, uint64_t scan_piece);

// sizing, a wave per chunk: text bytes of the chunk's tokens and its summed label (segment) lengths; with a translation also whether a
// position of the chunk fits no segment
void launch_chunk_stats(const ChunkedRows &r, const uint32_t *d_label_len, uint64_t n_labels, uint32_t first_node, int p_lines, uint64_t *d_chunk_text, uint64_t *d_chunk_seq,
                        hipStream_t s);
void launch_chunk_stats_segments(const ChunkedRows &r, const SegmentTables &t, int p_lines, uint64_t *d_chunk_text, uint64_t *d_chunk_seq, uint64_t *d_chunk_bad, hipStream_t s);
// per row the length of its line and its end coordinate: from the scans over the chunks (d_bad_before and d_valid null without a
// translation; a flagged line gets length 0), or from the line cache of the index
void launch_line_sizes(const uint64_t *d_seq_ids, const uint64_t *d_chunk_first, uint64_t n, const uint64_t *d_text_before, const uint64_t *d_seq_before,
                       const uint64_t *d_bad_before, const LineHeaders &hdr, int p_lines, uint64_t *d_line_len, uint64_t *d_line_end, uint8_t *d_valid, hipStream_t s);
void launch_line_sizes_cached(const uint64_t *d_offsets, const uint64_t *d_seq_ids, uint64_t n, const LineCache &cache, const LineHeaders &hdr, int p_lines, uint64_t *d_line_len,
                              uint64_t *d_line_end, hipStream_t s);
// formatting without a translation: what every chunk starts from (cache.text null: from d_text_before), then a workgroup per chunk
void launch_plan_chunks(const ChunkedRows &r, const uint64_t *d_text_before, int p_lines, const uint64_t *d_line_start, const uint64_t *d_seq_ids, const LineHeaders &hdr,
                        const uint64_t *d_line_end, const LineCache &cache, ChunkPlan *d_plans, hipStream_t s);
void launch_format_chunks(const ChunkedRows &r, const ChunkPlan *d_plans, int p_lines, const uint64_t *d_seq_ids, const LineHeaders &hdr, const uint64_t *d_line_end,
                          uint8_t *d_out, hipStream_t s);
// formatting with a translation: a workgroup per chunk; the lines of flagged rows (d_valid[row] == 0) are left to the host
void launch_format_chunks_segments(const ChunkedRows &r, const uint64_t *d_text_before, const SegmentTables &t, int p_lines, const uint8_t *d_valid,
                                   const uint64_t *d_line_start, const uint64_t *d_seq_ids, const LineHeaders &hdr, const uint64_t *d_line_end, uint8_t *d_out, hipStream_t s);
// GBZ::segment_path as data: tokens and flag per chunk, tokens and validity per row from their scans, the tokens of the valid rows
void launch_segment_chunk_tokens(const ChunkedRows &r, const SegmentTables &t, uint64_t *d_chunk_tokens, uint64_t *d_chunk_bad, hipStream_t s);
void launch_segment_row_tokens(const uint64_t *d_chunk_first, uint64_t n, const uint64_t *d_tokens_before, const uint64_t *d_bad_before, uint64_t *d_row_tokens,
                               uint8_t *d_valid, hipStream_t s);
void launch_segment_fill_tokens(const ChunkedRows &r, const uint64_t *d_tokens_before, const SegmentTables &t, const uint8_t *d_valid, const uint64_t *d_row_start,
                                uint64_t *d_out, hipStream_t s);

}  // namespace gbwt_hip
