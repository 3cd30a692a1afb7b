// sequences.hpp -- launch wrappers of sequences.hip: the bases of a batch of extracted rows cut into the chunks of the line formatter
// (lines.hpp: ChunkedRows, launch_chunk_plan).  The label upload of a handle, which sequences.hip also holds, is declared in labels.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "labels.hpp"
#include "lines.hpp"

namespace gbwt_hip {

// What the workgroup of a chunk starts from: where its node ids and its bytes begin, how many positions it has, where the endmarker of
// its row goes when it is the row's last chunk (~0: nowhere).
struct __attribute__((aligned(16))) SeqPlan {
    uint64_t ids_at, out_at, endmarker_at;
    uint32_t count, reserved;
};
static_assert(sizeof(SeqPlan) == 32, "two 16-byte loads");

// Whether the bases kernel can take the longest label of the handle (after ensure_labels), and what a request is refused with otherwise
bool labels_fit_a_batch(const gbwt_hip_index *ix);
extern const char *const LABELS_TOO_LONG;

// sizing, a wave per chunk: the bases of the chunk's positions
void launch_chunk_bases(const ChunkedRows &r, const Labels &L, uint64_t *d_chunk_bases, hipStream_t s);
// bytes of every row: its bases -- from the line cache of the index (d_cache_path, or null: from the scan over the chunks) -- and the endmarker
void launch_row_bytes(const uint64_t *d_seq_ids, uint64_t n, uint64_t n_sequences, const uint64_t *d_cache_path, const uint64_t *d_chunk_first, const uint64_t *d_bases_before,
                      int endmarker, uint64_t *d_row_len, hipStream_t s);
// what every chunk starts from, then a workgroup per chunk
void launch_plan_bases(const ChunkedRows &r, const uint64_t *d_seq_ids, uint64_t n_sequences, const uint64_t *d_bases_before, const uint64_t *d_row_start, int endmarker,
                       SeqPlan *d_plans, hipStream_t s);
void launch_bases(const ChunkedRows &r, const SeqPlan *d_plans, const Labels &L, int endmarker, uint8_t *d_out, hipStream_t s);

}  // namespace gbwt_hip
