// fm_chains.hpp -- the colinear chains of a read's hits (include/gbwt_hip.h, "Chains of seeds") as kernels (fm_chains.hip) and a
// host program (tests/cpp/fm_chains.cpp) both see them: when a match may precede another, what joining them scores, the key one wave
// reduction picks the predecessor with, the walk that peels chains off, and the summary of a chain.  __host__ __device__, no HIP call, as
// fm_seeds.hpp.
//
// MATCHES of an item (one read on one strand), ordered by (y, x): y a text position, x the start in the read, w the length.  All of it is
// integer arithmetic; nothing is heuristic.
// PRECEDENCE.  j may precede i when both lie in one segment of the text, dy = y_i - y_j and dx = x_i - x_j are in 1 .. max_gap, and
// d = |dy - dx| <= max_skew.  The segments are stretches of the text and the matches ascend by y, so "same segment and dy <= max_gap" is
// y_j >= low(i) = max(y_i - max_gap, first position of i's segment): one number per i, and low never decreases with i.
// SCORES.  c(j, i) = f(j) + min(w_i, dx, dy) - gap_cost * d, signed.  f(i) = w_i without predecessor unless some c(j, i) > w_i: then the
// largest c, and the largest j that attains it.  A kept c is > w_i >= 1 and <= x_i + w_i, so (c << 32) | j orders exactly that way as u64
// and 0 stands for "none".
// PEELING.  The matches are visited by (f descending, index ascending); an unused one starts a chain and walks its predecessors, marking
// them used, until there is none (base 0) or the next one is used (base = its f; it is no member).  score = f(head) - base, which is
// below 1 where joining the used predecessor gained nothing: such a chain is never reported.
#pragma once

#include <cstdint>

#include "../../include/gbwt_hip.h"
#include "fm_layout.hpp"

namespace gbwt_hip {

constexpr uint32_t FM_CHAIN_NONE = 0xFFFFFFFFu;                // pred: no predecessor
constexpr uint32_t FM_CHAIN_DEFAULT_GAP = 5000, FM_CHAIN_DEFAULT_SKEW = 500;   // conventions of the options, not tuned values
constexpr uint64_t FM_CHAIN_MAX_OPTION = 0x7FFFFFFFull;        // max_gap, max_skew, and gap_cost * max_skew stay below 2^31

struct FmChainParams { uint32_t max_gap, max_skew, gap_cost, min_score; };

// The options as the arithmetic takes them: 0 for a gap or a skew is the convention, a min_score of 0 counts as 1
FM_HD FmChainParams fm_chain_params(uint32_t max_gap, uint32_t max_skew, uint32_t gap_cost, uint32_t min_score) {
    return FmChainParams{max_gap == 0 ? FM_CHAIN_DEFAULT_GAP : max_gap, max_skew == 0 ? FM_CHAIN_DEFAULT_SKEW : max_skew, gap_cost, min_score < 1 ? 1u : min_score};
}

// low(i): the smallest y a predecessor of a match at y in the segment that starts at seg_start may have
FM_HD uint32_t fm_chain_low(uint32_t y, uint32_t seg_start, uint32_t max_gap) {
    const uint32_t by_gap = y > max_gap ? y - max_gap : 0;
    return by_gap > seg_start ? by_gap : seg_start;
}

// May j precede i?  low_i = fm_chain_low of i.  dx, dy, d are set where it may
FM_HD bool fm_chain_admissible(uint32_t yj, uint32_t xj, uint32_t yi, uint32_t xi, uint32_t low_i, const FmChainParams &P, uint32_t &dx, uint32_t &dy, uint32_t &d) {
    if (yj < low_i || yj >= yi || xj >= xi) return false;
    dy = yi - yj;
    dx = xi - xj;
    if (dx > P.max_gap) return false;
    d = dy > dx ? dy - dx : dx - dy;
    return d <= P.max_skew;
}

FM_HD int64_t fm_chain_score(uint32_t fj, uint32_t wi, uint32_t dx, uint32_t dy, uint32_t d, uint32_t gap_cost) {
    const uint32_t least = dx < dy ? dx : dy;
    return static_cast<int64_t>(fj) + (wi < least ? wi : least) - static_cast<int64_t>(gap_cost) * d;
}

// One candidate j of i against the best key so far (0: none); *pairs counts the admissible ones
FM_HD uint64_t fm_chain_step(uint64_t best, uint32_t j, uint32_t yj, uint32_t xj, uint32_t fj, uint32_t yi, uint32_t xi, uint32_t wi, uint32_t low_i, const FmChainParams &P,
                             uint64_t &pairs) {
    uint32_t dx = 0, dy = 0, d = 0;
    if (!fm_chain_admissible(yj, xj, yi, xi, low_i, P, dx, dy, d)) return best;
    pairs++;
    const int64_t c = fm_chain_score(fj, wi, dx, dy, d, P.gap_cost);
    if (c <= static_cast<int64_t>(wi)) return best;
    const uint64_t key = (static_cast<uint64_t>(c) << 32) | j;
    return key > best ? key : best;
}

// f(i) and pred(i) from the largest key over all j
FM_HD void fm_chain_result(uint64_t best, uint32_t wi, uint32_t &f, uint32_t &pred) {
    f = best != 0 ? static_cast<uint32_t>(best >> 32) : wi;
    pred = best != 0 ? static_cast<uint32_t>(best) : FM_CHAIN_NONE;
}

// The key of the stable sort that gives the visiting order of the peeling: items ascending, f descending; the sort keeps indices ascending
FM_HD uint64_t fm_chain_visit_key(uint64_t item, uint32_t f) { return (item << 32) | (0xFFFFFFFFu - f); }

// The walk from an unused head (an index into the item's f / pred / used / slot / pos): members are marked used, get the chain's visiting
// slot and their distance from the head.  Returns the members; score and tail (the last member, the smallest index) are set.
template <class Used>
FM_HD uint32_t fm_chain_peel(uint32_t head, uint32_t slot, const uint32_t *f, const uint32_t *pred, Used *used, uint32_t *member_slot, uint32_t *member_pos, int64_t &score,
                             uint32_t &tail) {
    uint32_t members = 0, at = head, base = 0;
    for (;;) {
        used[at] = 1;
        member_slot[at] = slot;
        member_pos[at] = members++;
        tail = at;
        const uint32_t p = pred[at];
        if (p == FM_CHAIN_NONE) break;
        if (used[p]) { base = f[p]; break; }
        at = p;
    }
    score = static_cast<int64_t>(f[head]) - base;       // behind a used predecessor the gain may be nothing or less: signed
    return members;
}

FM_HD bool fm_chain_reported(int64_t score, const FmChainParams &P) { return score >= static_cast<int64_t>(P.min_score); }

// The row of a chain from its first (tail) and last (head) member
FM_HD gbwt_hip_fm_chain fm_chain_summary(uint32_t y_first, uint32_t x_first, uint32_t y_last, uint32_t x_last, uint32_t w_last, uint32_t score, uint32_t members, uint32_t strand,
                                         uint32_t path) {
    return gbwt_hip_fm_chain{y_first, static_cast<uint64_t>(y_last) + w_last, x_first, x_last + w_last, score, members, strand, path};
}

}  // namespace gbwt_hip
