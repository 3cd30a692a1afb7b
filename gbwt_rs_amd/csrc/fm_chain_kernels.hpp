// fm_chain_kernels.hpp -- the kernels of the chaining behind a seeds request (fm_chains.hip) as the C ABI launches them (capi_fm_chains.hip).
// What a match, a predecessor and a chain are is fm_chains.hpp; the sizes of the buffers are fm_chain_plan.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/gbwt_hip.h"
#include "fm_chains.hpp"

namespace gbwt_hip {

// The rows of the seeds step and the arrays the chaining passes on.  ITEMS, read-major: item q = read q / ns on the (q % ns)-th strand of
// the request (ns strands), which is the order of the seeds rows and of the chain rows.  MATCHES of item q: [match_offsets[q],
// match_offsets[q + 1]), before the first sort in seed and hit order, behind it by (y, x).  VISITING SLOTS: the same stretch in peeling order.
struct ChainBatch {
    // the seeds step
    const uint64_t *seed_read_offsets;        // [m + 1]
    const gbwt_hip_fm_seed *seeds;            // [total_seeds]
    const uint64_t *hit_offsets;              // [total_seeds + 1]
    const uint64_t *positions;                // [total_hits]
    uint64_t m, total_seeds, total_hits;
    uint32_t strands, ns;
    // the segments: the text offsets of the paths [n_paths + 1], or null on an index of a plain text
    const uint64_t *path_offsets;
    uint64_t n_paths;
    FmChainParams P;
    uint64_t max_matches;
    uint64_t items, matches;
    uint64_t *counts, *match_offsets, *hit_first;              // [items], [items + 1], [items + 1]
    uint64_t *key_a, *val_a, *key_b, *val_b;                   // [hits] each
    uint32_t *y, *x, *w, *low, *seg, *f, *pred;                // [hits] each; pred counts from the item's first match
    uint8_t *used;                                             // [hits]
    uint32_t *member_slot, *member_pos, *slot_score, *slot_tail;
    uint64_t *flags, *rank, *members, *member_rank;            // [hits], [hits + 1], [hits], [hits + 1]
    uint64_t *words;                                           // [0] += skipped items, [1] += pairs
};

// the visiting order reuses the buffers of the first sort: keys in key_a, sorted into val_a; indices and the order in the halves of val_b
inline uint32_t *chain_visit_index(const ChainBatch &b) { return reinterpret_cast<uint32_t *>(b.val_b); }
inline uint32_t *chain_visit_order(const ChainBatch &b) { return reinterpret_cast<uint32_t *>(b.val_b) + b.matches; }

// the temporary storage of the two sorts over `hits` pairs, with hipcub's status
hipError_t chain_sort_temp_bytes(uint64_t hits, uint64_t items, size_t &bytes);

// counts[q] = the hits of item q (0 and a skipped item where they exceed max_matches), hit_first[q] = its first hit ([items]: all hits)
void launch_chain_item_counts(const ChainBatch &b, hipStream_t s);
// Behind the scan of the counts: one lane per match writes key_a = item << 32 | y and val_a = x << 32 | w, in seed and hit order
void launch_chain_expand(const ChainBatch &b, hipStream_t s);
// The stable sort by (item, y) into key_b / val_b, and y, x, w, low and the segment of every match out of them.  The sorts return hipcub's
// status, and hipErrorInvalidValue where the temporary storage is less than hipcub asks for the matches
hipError_t launch_chain_sort_matches(const ChainBatch &b, void *d_temp, size_t temp_bytes, hipStream_t s);
// The DP: one wave per item; f and pred of every match, the pairs into words[1]
void launch_chain_dp(const ChainBatch &b, hipStream_t s);
// The visiting order: keys from f, the stable sort, and the order of every slot
hipError_t launch_chain_sort_visits(const ChainBatch &b, void *d_temp, size_t temp_bytes, hipStream_t s);
// One lane per item walks its slots: per match the slot of its chain and its distance from the head; per slot that heads a chain its score
// and tail, flags = 1 and members = their number where it is reported, else 0
void launch_chain_peel(const ChainBatch &b, hipStream_t s);
// Behind the scans of flags and members: the chains, their match offsets [chains + 1], their members, and the offsets of the reads' rows [m + 1]
void launch_chain_fill(const ChainBatch &b, uint64_t total_chains, uint64_t *d_read_offsets, gbwt_hip_fm_chain *d_chains, uint64_t *d_chain_match_offsets,
                       gbwt_hip_fm_chain_match *d_matches, hipStream_t s);

}  // namespace gbwt_hip
