// gfa_parse.hip -- GFA text to rows of nodes and node labels on the device: the inverse of the line formatter of lines.hip.
//
// Count, scan, fill -- no lane loops over a line.  The text is cut into tiles of GFA_TILE_BYTES, one wave per tile, 16 bytes per lane.
//   structure  k_gfa_count_structure / k_gfa_record_structure: the positions of every '\n' and '\t' (tile counts, a scan, a fill);
//              k_gfa_lines: one thread per line -- its kind, its fields (a bisection into the tabs) and its step field or sequence;
//              scans of the kind flags rank the H-, S-, P- and W-lines; k_gfa_gather_lines lists them.
//   steps      k_gfa_count_steps: a tile knows its first line (the newlines in front of it: the scan), takes the step fields that cross it
//              and counts their orientation marks ('+' '-' in a P-line, '>' '<' in a W-line: with integer names nothing else in the field
//              can be one); a scan per kind; k_gfa_fill_steps: one lane per mark reads the (at most 10) digits of its token -- behind the
//              mark in a W-line, in front of it in a P-line, across a tile edge if need be --, checks them, looks the id up in the bit table
//              of the S-lines and stores 2 * id + reverse.  The tile that holds the first byte of a step field writes the path's row offset.
//              Path order is "P-lines, then W-lines", so the two kinds are counted apart and the W rows lie behind the P rows.
//   labels     a radix sort of the S ids finds the duplicates; the S-lines of visited nodes fill a dense table of (length, source), a scan
//              gives the offsets, k_gfa_copy_labels copies, split by output bytes.
// Refusals go through one error word, (line << 8 | code), lowered with atomicMin.
//
// A translated parse (segment names that are no node ids, long segments chopped; the rules are in include/gbwt_hip.h) keeps that shape:
//   names      k_gfa_segment_plan: one lane per S-line -- the hash of its name (gfa_names.hpp) and the number of its nodes; a scan gives the
//              first node of every segment; a radix sort of (hash, S rank), k_gfa_name_duplicates over the runs of equal hashes,
//              k_gfa_name_buckets: one bisection per bucket of the top bits.
//   steps      k_gfa_count_tokens / k_gfa_fill_tokens: the marks of a P-line are the token STARTS (a name may hold '+' or '-'); one lane per
//              token finds its end, looks the name up and stores (segment, orientation) and the segment's node count.
//   expand     a scan of the node counts; k_gfa_expand_steps: one lane per output node bisects it for its step -- a step on a segment of
//              four million bases and one on a single base take the same path.
//   labels     k_gfa_node_slots: the (length, source) table is per NODE, a chunk of its segment's sequence; the names of the visited
//              segments come back through the same copy (k_gfa_name_slots).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>

#include "build.hpp"
#include "capi_internal.hpp"
#include "device_common.hpp"
#include "gfa_names.hpp"
#include "gfa_parse.hpp"

namespace gbwt_hip {

namespace {

constexpr int THREADS = 256;
constexpr uint32_t WAVES = THREADS / 64;
static_assert(GFA_TILE_BYTES == 64 * 16, "a tile is one 16-byte load of every lane of a wave");

enum LineKind : uint8_t { KIND_EMPTY = 0, KIND_H, KIND_S, KIND_L, KIND_P, KIND_W, KIND_IGNORED, KIND_BAD };
enum Counter : uint32_t { CNT_LINES = 0, CNT_H, CNT_S, CNT_L, CNT_P, CNT_W, CNT_IGNORED, CNT_LABEL_BYTES, CNT_MAX_ID, CNT_GRAPH_NODES, CNT_NOT_ID, CNT_MAX_SEQUENCE, CNT_CHOPPED, CNT_WORDS };

using u64 = unsigned long long;

__device__ __forceinline__ void post(u64 *err, uint64_t line, uint32_t code) { atomicMin(err, (static_cast<u64>(line) << 8) | code); }

// bit i = byte i of the word equals the byte repeated in c4
__device__ __forceinline__ uint32_t eq_mask4(uint32_t w, uint32_t c4) {
    const uint32_t x = w ^ c4;
    const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
    return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}
__device__ __forceinline__ uint32_t eq_mask16(const uint4 &v, uint8_t c) {
    const uint32_t c4 = c * 0x01010101u;
    return eq_mask4(v.x, c4) | (eq_mask4(v.y, c4) << 4) | (eq_mask4(v.z, c4) << 8) | (eq_mask4(v.w, c4) << 12);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// (every lane of the wave must be here)
__device__ __forceinline__ uint32_t wave_exclusive(uint32_t v, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= static_cast<uint32_t>(d)) x += y;
    }
    total = __shfl(x, 63, 64);
    return x - v;
}

__device__ __forceinline__ uint4 load_tile(const uint8_t *text, uint64_t tile) {
    return *reinterpret_cast<const uint4 *>(text + tile * GFA_TILE_BYTES + (threadIdx.x & 63) * 16);
}

// ---- structure -------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void k_gfa_count_structure(const uint8_t *__restrict__ text, uint64_t tiles, uint64_t *__restrict__ tile_nl, uint64_t *__restrict__ tile_tab) {
    const uint64_t tile = static_cast<uint64_t>(blockIdx.x) * WAVES + threadIdx.x / 64;
    if (tile >= tiles) return;
    const uint4 v = load_tile(text, tile);
    const uint32_t nl = wave_sum(__popc(eq_mask16(v, '\n'))), tab = wave_sum(__popc(eq_mask16(v, '\t')));
    if ((threadIdx.x & 63) == 0) { tile_nl[tile] = nl; tile_tab[tile] = tab; }
}

// tile_nl / tile_tab: scanned (the newlines / tabs in front of the tile)
__global__ __launch_bounds__(THREADS) void k_gfa_record_structure(const uint8_t *__restrict__ text, uint64_t tiles, const uint64_t *__restrict__ tile_nl,
                                                                  const uint64_t *__restrict__ tile_tab, uint64_t *__restrict__ nl_pos, uint64_t *__restrict__ tab_pos, u64 *err) {
    const uint64_t tile = static_cast<uint64_t>(blockIdx.x) * WAVES + threadIdx.x / 64;
    if (tile >= tiles) return;
    const uint4 v = load_tile(text, tile);
    const uint64_t p0 = tile * GFA_TILE_BYTES + (threadIdx.x & 63) * 16;
    const uint32_t nl = eq_mask16(v, '\n'), tab = eq_mask16(v, '\t'), cr = eq_mask16(v, '\r');
    uint32_t total;
    const uint64_t nl_at = tile_nl[tile] + wave_exclusive(__popc(nl), total);
    const uint64_t tab_at = tile_tab[tile] + wave_exclusive(__popc(tab), total);
    uint32_t k = 0;
    for (uint32_t m = nl; m; m &= m - 1) nl_pos[nl_at + k++] = p0 + (__ffs(m) - 1);
    k = 0;
    for (uint32_t m = tab; m; m &= m - 1) tab_pos[tab_at + k++] = p0 + (__ffs(m) - 1);
    if (cr) post(err, nl_at + __popc(nl & ((1u << (__ffs(cr) - 1)) - 1u)), GFA_ERR_CR);
}

struct LineTables {
    uint8_t *kind;          // [lines]
    uint64_t *first_tab;    // index of the line's first tab in tab_pos
    uint64_t *lo, *hi;      // the step field of a P- / W-line, the sequence of an S-line
    uint32_t *id;           // the node id of an S-line
    uint32_t *rank_h, *rank_s, *rank_p, *rank_w;   // flags, then (scanned) ranks among the lines of the kind
};

// a decimal node id: 1 .. 10 digits, no leading zero, 1 .. 2^31 - 1
__device__ __forceinline__ bool parse_id(const uint8_t *text, uint64_t lo, uint64_t hi, uint32_t &id) {
    if (hi <= lo || hi - lo > 10 || text[lo] == '0') return false;
    uint64_t v = 0;
    for (uint64_t i = lo; i < hi; i++) {
        const uint32_t d = static_cast<uint32_t>(text[i]) - '0';
        if (d > 9) return false;
        v = v * 10 + d;
    }
    if (v == 0 || v > 0x7FFFFFFFull) return false;
    id = static_cast<uint32_t>(v);
    return true;
}

__global__ __launch_bounds__(THREADS) void k_gfa_lines(const uint8_t *__restrict__ text, const uint64_t *__restrict__ nl_pos, uint64_t lines, const uint64_t *__restrict__ tab_pos,
                                                       uint64_t tabs, LineTables t, uint32_t names, u64 *counters, u64 *err) {
    const uint64_t l = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (l >= lines) return;
    const uint64_t start = l ? nl_pos[l - 1] + 1 : 0, end = nl_pos[l];
    uint8_t kind = KIND_EMPTY;
    uint64_t lo = 0, hi = 0, ft = 0;
    uint32_t id = 0;
    bool not_id = false;
    if (end > start) {
        ft = lower_bound(tab_pos, 0, tabs, start);
        const uint64_t nt = lower_bound(tab_pos, ft, tabs, end) - ft;
        const auto field_lo = [&](uint64_t k) { return tab_pos[ft + k - 1] + 1; };                       // k >= 1, k <= nt
        const auto field_hi = [&](uint64_t k) { return k < nt ? tab_pos[ft + k] : end; };
        const bool tagged = nt >= 1 && tab_pos[ft] == start + 1;                                           // the kind is a field of one byte
        switch (text[start]) {
            case 'H': kind = KIND_H; break;
            case 'S':
                kind = KIND_BAD;
                if (!tagged || nt < 2) { post(err, l, GFA_ERR_MALFORMED); break; }
                if (names) {                                                                                 // any 1 .. GFA_MAX_NAME bytes; whether it is a node id decides AUTO
                    const uint64_t n_lo = field_lo(1), n_hi = field_hi(1);
                    not_id = !parse_id(text, n_lo, n_hi, id);
                    if (not_id) id = 0;
                    if (n_hi == n_lo) { post(err, l, GFA_ERR_EMPTY_NAME); break; }
                    if (n_hi - n_lo > GFA_MAX_NAME) { post(err, l, GFA_ERR_LONG_NAME); break; }
                } else if (!parse_id(text, field_lo(1), field_hi(1), id)) { post(err, l, GFA_ERR_NAME); break; }
                lo = field_lo(2); hi = field_hi(2);
                if (hi == lo || (hi == lo + 1 && text[lo] == '*')) { post(err, l, GFA_ERR_SEQUENCE); break; }
                kind = KIND_S;
                break;
            case 'L':
                if (!tagged || nt < 4) { kind = KIND_BAD; post(err, l, GFA_ERR_MALFORMED); } else kind = KIND_L;
                break;
            case 'P':
                if (!tagged || nt < 2) { kind = KIND_BAD; post(err, l, GFA_ERR_MALFORMED); break; }
                kind = KIND_P; lo = field_lo(2); hi = field_hi(2);
                break;
            case 'W':
                if (!tagged || nt < 6) { kind = KIND_BAD; post(err, l, GFA_ERR_MALFORMED); break; }
                kind = KIND_W; lo = field_lo(6); hi = field_hi(6);
                break;
            default: kind = KIND_IGNORED;
        }
        if ((kind == KIND_P || kind == KIND_W) && hi == lo + 1 && text[lo] == '*') hi = lo;                // "*": no steps
        if (kind == KIND_BAD) { lo = 0; hi = 0; }
    }
    t.kind[l] = kind; t.first_tab[l] = ft; t.lo[l] = lo; t.hi[l] = hi; t.id[l] = id;
    t.rank_h[l] = kind == KIND_H; t.rank_s[l] = kind == KIND_S; t.rank_p[l] = kind == KIND_P; t.rank_w[l] = kind == KIND_W;
    // (one add per wave and address: the compiler sums the active lanes)
    if (kind != KIND_EMPTY) atomicAdd(&counters[CNT_LINES], 1ull);
    if (kind == KIND_H) atomicAdd(&counters[CNT_H], 1ull);
    if (kind == KIND_S) { atomicAdd(&counters[CNT_S], 1ull); atomicAdd(&counters[CNT_LABEL_BYTES], static_cast<u64>(hi - lo)); atomicMax(&counters[CNT_MAX_ID], static_cast<u64>(id)); }
    if (kind == KIND_S && names) atomicMax(&counters[CNT_MAX_SEQUENCE], static_cast<u64>(hi - lo));
    if (not_id) atomicAdd(&counters[CNT_NOT_ID], 1ull);
    if (kind == KIND_L) atomicAdd(&counters[CNT_L], 1ull);
    if (kind == KIND_P) atomicAdd(&counters[CNT_P], 1ull);
    if (kind == KIND_W) atomicAdd(&counters[CNT_W], 1ull);
    if (kind == KIND_IGNORED) atomicAdd(&counters[CNT_IGNORED], 1ull);
}

// The lines of a kind, listed: [start, end) of the H-lines; id and line of the S-lines, with their bit in the presence table; line and
// tabs of the paths (the P-lines, then the W-lines)
__global__ __launch_bounds__(THREADS) void k_gfa_gather_lines(const uint64_t *__restrict__ nl_pos, uint64_t lines, const uint64_t *__restrict__ tab_pos, LineTables t, uint64_t n_p,
                                                              uint64_t *__restrict__ headers, uint32_t *__restrict__ seg_id, uint32_t *__restrict__ seg_line,
                                                              uint32_t *__restrict__ present, GfaPathLine *__restrict__ paths) {
    const uint64_t l = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (l >= lines) return;
    const uint8_t kind = t.kind[l];
    if (kind == KIND_H) {
        headers[2 * t.rank_h[l]] = l ? nl_pos[l - 1] + 1 : 0;
        headers[2 * t.rank_h[l] + 1] = nl_pos[l];
    } else if (kind == KIND_S) {
        const uint32_t id = t.id[l];
        seg_id[t.rank_s[l]] = id; seg_line[t.rank_s[l]] = static_cast<uint32_t>(l);
        if (present) atomicOr(&present[id >> 5], 1u << (id & 31));       // (a translated parse has no table over the ids)
    } else if (kind == KIND_P || kind == KIND_W) {
        GfaPathLine p;
        p.line = l; p.walk = kind == KIND_W;
        const uint32_t n = kind == KIND_W ? 6 : 2;
        for (uint32_t k = 0; k < 6; k++) p.tab[k] = k < n ? tab_pos[t.first_tab[l] + k] : 0;
        paths[kind == KIND_W ? n_p + t.rank_w[l] : t.rank_p[l]] = p;
    }
}

// ---- steps -----------------------------------------------------------------------------------------------------------------------------

// bits of the lane's 16 bytes at p0 that lie in [lo, hi)
__device__ __forceinline__ uint32_t range_mask(uint64_t p0, uint64_t lo, uint64_t hi) {
    const uint32_t from = lo > p0 ? static_cast<uint32_t>(lo - p0 < 16 ? lo - p0 : 16) : 0;
    const uint32_t to = hi > p0 ? static_cast<uint32_t>(hi - p0 < 16 ? hi - p0 : 16) : 0;
    return to > from ? ((1u << to) - 1u) & ~((1u << from) - 1u) : 0u;
}

// Lines first .. last cross the tile: `first` has as many newlines in front of it as the tile, `last` starts behind the tile's last newline
__device__ __forceinline__ void tile_lines(const uint64_t *tile_nl, uint64_t tile, uint64_t tiles, uint64_t lines, uint64_t &first, uint64_t &last) {
    first = tile_nl[tile];
    last = tile + 1 < tiles ? tile_nl[tile + 1] : lines;
    if (last >= lines) last = lines - 1;
}

__global__ __launch_bounds__(THREADS) void k_gfa_count_steps(const uint8_t *__restrict__ text, uint64_t tiles, const uint64_t *__restrict__ tile_nl, uint64_t lines, LineTables t,
                                                             uint64_t *__restrict__ tile_p, uint64_t *__restrict__ tile_w) {
    const uint64_t tile = static_cast<uint64_t>(blockIdx.x) * WAVES + threadIdx.x / 64;
    if (tile >= tiles) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t a = tile * GFA_TILE_BYTES, b = a + GFA_TILE_BYTES, p0 = a + lane * 16;
    const uint4 v = load_tile(text, tile);
    const uint32_t marks_p = eq_mask16(v, '+') | eq_mask16(v, '-'), marks_w = eq_mask16(v, '>') | eq_mask16(v, '<');
    uint32_t count_p = 0, count_w = 0;
    uint64_t first, last;
    tile_lines(tile_nl, tile, tiles, lines, first, last);
    if (first < lines)
        for (uint64_t base = first; base <= last; base += 64) {
            const uint64_t l = base + lane;
            const uint8_t kind = l <= last ? t.kind[l] : KIND_EMPTY;
            const bool path = kind == KIND_P || kind == KIND_W;
            const uint64_t lo = path ? t.lo[l] : 0, hi = path ? t.hi[l] : 0;
            for (uint64_t m = __ballot(path && hi > lo && lo < b && hi > a); m; m &= m - 1) {
                const int j = __ffsll(static_cast<u64>(m)) - 1;
                const uint32_t in_field = range_mask(p0, shfl64(lo, j), shfl64(hi, j));
                if (__shfl(static_cast<uint32_t>(kind), j, 64) == KIND_W) count_w += __popc(marks_w & in_field); else count_p += __popc(marks_p & in_field);
            }
        }
    count_p = wave_sum(count_p); count_w = wave_sum(count_w);
    if (lane == 0) { tile_p[tile] = count_p; tile_w[tile] = count_w; }
}

__device__ __forceinline__ bool is_digit(uint8_t c) { return static_cast<uint32_t>(c) - '0' <= 9; }

// The token of the mark at q of a step field [lo, hi).  W: ">id" / "<id", the id behind the mark up to the next mark or the end of the
// field.  P: "id+" / "id-", the id in front of the mark back to the start of the field or a ',' behind a mark; behind the mark the end of
// the field or a ','.  Every byte read lies in [lo, hi] (hi is the tab or newline behind the field).
__device__ __forceinline__ bool parse_step(const uint8_t *text, uint64_t lo, uint64_t hi, uint64_t q, bool walk, uint32_t &id) {
    uint64_t v = 0;
    uint32_t d = 0;
    if (walk) {
        uint64_t pos = q + 1;
        while (pos < hi && d < 11 && is_digit(text[pos])) { v = v * 10 + (text[pos] - '0'); d++; pos++; }
        if (d < 1 || d > 10 || text[q + 1] == '0') return false;
        if (pos != hi && text[pos] != '>' && text[pos] != '<') return false;
    } else {
        uint64_t pos = q, unit = 1;
        while (pos > lo && d < 11 && is_digit(text[pos - 1])) { v += unit * (text[pos - 1] - '0'); unit *= 10; d++; pos--; }
        if (d < 1 || d > 10 || text[pos] == '0') return false;
        if (pos != lo && !(text[pos - 1] == ',' && pos >= lo + 2 && (text[pos - 2] == '+' || text[pos - 2] == '-'))) return false;
        if (q + 1 != hi && text[q + 1] != ',') return false;
    }
    if (v == 0 || v > 0x7FFFFFFFull) return false;
    id = static_cast<uint32_t>(v);
    return true;
}

// tile_p / tile_w: scanned.  offsets[path] and nodes[] as documented at the top; visited: a bit per node id some step names.
__global__ __launch_bounds__(THREADS) void k_gfa_fill_steps(const uint8_t *__restrict__ text, uint64_t tiles, const uint64_t *__restrict__ tile_nl, uint64_t lines, LineTables t,
                                                            const uint64_t *__restrict__ tile_p, const uint64_t *__restrict__ tile_w, uint64_t n_p, uint64_t steps_p,
                                                            const uint32_t *__restrict__ present, uint64_t max_id, uint32_t *__restrict__ visited, uint64_t *__restrict__ offsets,
                                                            uint32_t *__restrict__ nodes, u64 *err) {
    const uint64_t tile = static_cast<uint64_t>(blockIdx.x) * WAVES + threadIdx.x / 64;
    if (tile >= tiles) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t a = tile * GFA_TILE_BYTES, b = a + GFA_TILE_BYTES, p0 = a + lane * 16;
    const uint4 v = load_tile(text, tile);
    const uint32_t marks_p = eq_mask16(v, '+') | eq_mask16(v, '-'), marks_w = eq_mask16(v, '>') | eq_mask16(v, '<');
    uint64_t done_p = tile_p[tile], done_w = steps_p + tile_w[tile];      // rows: the steps of the P-lines, then those of the W-lines
    uint64_t first, last;
    tile_lines(tile_nl, tile, tiles, lines, first, last);
    if (first >= lines) return;
    for (uint64_t base = first; base <= last; base += 64) {
        const uint64_t l = base + lane;
        const uint8_t kind = l <= last ? t.kind[l] : KIND_EMPTY;
        const bool path = kind == KIND_P || kind == KIND_W;
        const uint64_t lo = path ? t.lo[l] : 0, hi = path ? t.hi[l] : 0;
        const uint64_t row = !path ? 0 : (kind == KIND_W ? n_p + t.rank_w[l] : t.rank_p[l]);
        // (a field without steps still has a first byte -- the tab or newline behind it -- whose tile writes the row offset)
        for (uint64_t m = __ballot(path && lo < b && (hi > lo ? hi : lo + 1) > a); m; m &= m - 1) {
            const int j = __ffsll(static_cast<u64>(m)) - 1;
            const uint64_t f_lo = shfl64(lo, j), f_hi = shfl64(hi, j), f_row = shfl64(row, j), f_line = base + j;
            const bool walk = __shfl(static_cast<uint32_t>(kind), j, 64) == KIND_W;
            const uint32_t mine = (walk ? marks_w : marks_p) & range_mask(p0, f_lo, f_hi);
            uint32_t total;
            const uint64_t at = (walk ? done_w : done_p) + wave_exclusive(__popc(mine), total);
            if (lane == 0) {
                if (f_lo >= a) offsets[f_row] = walk ? done_w : done_p;
                if (f_hi > f_lo) {
                    // the ends that no mark's token covers: a walk starts with a mark, a list of steps ends with one
                    if (walk && f_lo >= a && text[f_lo] != '>' && text[f_lo] != '<') post(err, f_line, GFA_ERR_STEP);
                    if (!walk && f_hi - 1 >= a && f_hi - 1 < b && text[f_hi - 1] != '+' && text[f_hi - 1] != '-') post(err, f_line, GFA_ERR_STEP);
                }
            }
            uint32_t k = 0;
            for (uint32_t mm = mine; mm; mm &= mm - 1, k++) {
                const uint64_t q = p0 + (__ffs(mm) - 1);
                uint32_t id = 0, node = 0;
                if (!parse_step(text, f_lo, f_hi, q, walk, id)) post(err, f_line, GFA_ERR_STEP);
                else if (id > max_id || !((present[id >> 5] >> (id & 31)) & 1u)) post(err, f_line, GFA_ERR_UNKNOWN_SEGMENT);
                else {
                    node = 2 * id + (text[q] == '<' || text[q] == '-');
                    if (!((visited[id >> 5] >> (id & 31)) & 1u)) atomicOr(&visited[id >> 5], 1u << (id & 31));
                }
                nodes[at + k] = node;
            }
            if (walk) done_w += total; else done_p += total;
        }
    }
}


// ---- translated: names ------------------------------------------------------------------------------------------------------------------

// One lane per S-line (by rank): where its name lies, the hash of the name and the number of nodes the segment owns
__global__ __launch_bounds__(THREADS) void k_gfa_segment_plan(const uint8_t *__restrict__ text, const uint64_t *__restrict__ tab_pos, LineTables t, const uint32_t *__restrict__ seg_line,
                                                              uint64_t n, uint32_t max_node_length, uint64_t *__restrict__ name_lo, uint32_t *__restrict__ name_len,
                                                              uint64_t *__restrict__ hash, uint32_t *__restrict__ rank, uint64_t *__restrict__ seg_nodes, u64 *counters) {
    const uint64_t k = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (k >= n) return;
    const uint64_t l = seg_line[k], ft = t.first_tab[l], lo = tab_pos[ft] + 1;
    uint32_t len = static_cast<uint32_t>(tab_pos[ft + 1] - lo);
    if (len > GFA_MAX_NAME) len = GFA_MAX_NAME;                               // (k_gfa_lines lets no such line become a segment)
    name_lo[k] = lo; name_len[k] = len; rank[k] = static_cast<uint32_t>(k);
    hash[k] = GfaNameHash()(text + lo, len);
    const uint64_t bases = t.hi[l] - t.lo[l];
    const uint64_t nodes = max_node_length ? (bases + max_node_length - 1) / max_node_length : 1;
    seg_nodes[k] = nodes ? nodes : 1;
    if (nodes > 1) atomicAdd(&counters[CNT_CHOPPED], 1ull);
}

// (hash, rank) sorted, the ranks of one hash ascending: an entry that names what an earlier entry of its run names is a later S-line of the name
__global__ __launch_bounds__(THREADS) void k_gfa_name_duplicates(GfaNameTable names, const uint32_t *__restrict__ seg_line, u64 *err) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (i == 0 || i >= names.segments) return;
    if (gfa_name_repeats(names, static_cast<uint32_t>(i))) post(err, seg_line[names.rank[i]], GFA_ERR_DUPLICATE_NAME);
}

// bucket[b]: the first sorted entry with the top bits >= b; one bisection per bucket
__global__ __launch_bounds__(THREADS) void k_gfa_name_buckets(const uint64_t *__restrict__ hash, uint64_t n, uint32_t bits, uint32_t *__restrict__ bucket) {
    const uint64_t b = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x, buckets = uint64_t(1) << bits;
    if (b > buckets) return;
    bucket[b] = static_cast<uint32_t>(b == buckets ? n : lower_bound(hash, 0, n, gfa_bucket_floor(b, bits)));
}

// ---- translated: steps ------------------------------------------------------------------------------------------------------------------

// The token starts of a P-line among the lane's 16 bytes at p0: the bytes behind a ',' (the first byte of the field is the caller's)
__device__ __forceinline__ uint32_t starts_behind_commas(const uint8_t *text, const uint4 &v, uint64_t p0) {
    const uint32_t carry = p0 > 0 && text[p0 - 1] == ',';
    return ((eq_mask16(v, ',') << 1) | carry) & 0xFFFFu;
}
__device__ __forceinline__ uint32_t first_byte_bit(uint64_t p0, uint64_t lo, uint64_t hi) { return hi > lo && lo >= p0 && lo < p0 + 16 ? 1u << (lo - p0) : 0u; }

__global__ __launch_bounds__(THREADS) void k_gfa_count_tokens(const uint8_t *__restrict__ text, uint64_t tiles, const uint64_t *__restrict__ tile_nl, uint64_t lines, LineTables t,
                                                              uint64_t *__restrict__ tile_p, uint64_t *__restrict__ tile_w) {
    const uint64_t tile = static_cast<uint64_t>(blockIdx.x) * WAVES + threadIdx.x / 64;
    if (tile >= tiles) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t a = tile * GFA_TILE_BYTES, b = a + GFA_TILE_BYTES, p0 = a + lane * 16;
    const uint4 v = load_tile(text, tile);
    const uint32_t marks_p = starts_behind_commas(text, v, p0), marks_w = eq_mask16(v, '>') | eq_mask16(v, '<');
    uint32_t count_p = 0, count_w = 0;
    uint64_t first, last;
    tile_lines(tile_nl, tile, tiles, lines, first, last);
    if (first < lines)
        for (uint64_t base = first; base <= last; base += 64) {
            const uint64_t l = base + lane;
            const uint8_t kind = l <= last ? t.kind[l] : KIND_EMPTY;
            const bool path = kind == KIND_P || kind == KIND_W;
            const uint64_t lo = path ? t.lo[l] : 0, hi = path ? t.hi[l] : 0;
            for (uint64_t m = __ballot(path && hi > lo && lo < b && hi > a); m; m &= m - 1) {
                const int j = __ffsll(static_cast<u64>(m)) - 1;
                const uint64_t f_lo = shfl64(lo, j), f_hi = shfl64(hi, j);
                const uint32_t in_field = range_mask(p0, f_lo, f_hi);
                if (__shfl(static_cast<uint32_t>(kind), j, 64) == KIND_W) count_w += __popc(marks_w & in_field);
                else count_p += __popc((marks_p & in_field) | first_byte_bit(p0, f_lo, f_hi));
            }
        }
    count_p = wave_sum(count_p); count_w = wave_sum(count_w);
    if (lane == 0) { tile_p[tile] = count_p; tile_w[tile] = count_w; }
}

// The token that starts at q of a step field [lo, hi).  W: ">name" / "<name", the name up to the next mark or the end of the field.
// P: "name+" / "name-", up to the next ',' or the end of the field; the orientation is its last byte.  The search for the end is bounded
// by the longest name: a longer token names no segment.  0, or the code of the refusal.
__device__ __forceinline__ uint32_t parse_named_step(const uint8_t *text, uint64_t lo, uint64_t hi, uint64_t q, bool walk, const GfaNameTable &names, uint32_t &segment, uint32_t &reverse) {
    uint64_t n_lo, n_hi;
    if (walk) {
        n_lo = q + 1;
        uint64_t e = n_lo;
        while (e < hi && e - n_lo <= GFA_MAX_NAME && text[e] != '>' && text[e] != '<') e++;
        if (e == n_lo) return GFA_ERR_NAMED_STEP;
        n_hi = e;
        reverse = text[q] == '<';
    } else {
        n_lo = q;
        uint64_t e = q;
        while (e < hi && e - q <= GFA_MAX_NAME + 1 && text[e] != ',') e++;
        if (e - q > GFA_MAX_NAME + 1) return GFA_ERR_UNKNOWN_SEGMENT;
        if (e - q < 2 || (text[e - 1] != '+' && text[e - 1] != '-')) return GFA_ERR_NAMED_STEP;
        n_hi = e - 1;
        reverse = text[e - 1] == '-';
    }
    if (n_hi - n_lo > GFA_MAX_NAME) return GFA_ERR_UNKNOWN_SEGMENT;
    segment = gfa_lookup_name(names, text + n_lo, static_cast<uint32_t>(n_hi - n_lo), GfaNameHash());
    return segment == GFA_NO_SEGMENT ? GFA_ERR_UNKNOWN_SEGMENT : 0u;
}

// tile_p / tile_w: scanned.  step_off[path]: the first step of the path; step_seg[]: 2 * segment + reverse; step_nodes[]: the nodes of the
// segment (seg_start: scanned); visited: a bit per segment some step names.
__global__ __launch_bounds__(THREADS) void k_gfa_fill_tokens(const uint8_t *__restrict__ text, uint64_t tiles, const uint64_t *__restrict__ tile_nl, uint64_t lines, LineTables t,
                                                             const uint64_t *__restrict__ tile_p, const uint64_t *__restrict__ tile_w, uint64_t n_p, uint64_t steps_p, GfaNameTable names,
                                                             const uint64_t *__restrict__ seg_start, uint32_t *__restrict__ visited, uint64_t *__restrict__ step_off,
                                                             uint32_t *__restrict__ step_seg, uint64_t *__restrict__ step_nodes, u64 *err) {
    const uint64_t tile = static_cast<uint64_t>(blockIdx.x) * WAVES + threadIdx.x / 64;
    if (tile >= tiles) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t a = tile * GFA_TILE_BYTES, b = a + GFA_TILE_BYTES, p0 = a + lane * 16;
    const uint4 v = load_tile(text, tile);
    const uint32_t marks_p = starts_behind_commas(text, v, p0), marks_w = eq_mask16(v, '>') | eq_mask16(v, '<');
    uint64_t done_p = tile_p[tile], done_w = steps_p + tile_w[tile];
    uint64_t first, last;
    tile_lines(tile_nl, tile, tiles, lines, first, last);
    if (first >= lines) return;
    for (uint64_t base = first; base <= last; base += 64) {
        const uint64_t l = base + lane;
        const uint8_t kind = l <= last ? t.kind[l] : KIND_EMPTY;
        const bool path = kind == KIND_P || kind == KIND_W;
        const uint64_t lo = path ? t.lo[l] : 0, hi = path ? t.hi[l] : 0;
        const uint64_t row = !path ? 0 : (kind == KIND_W ? n_p + t.rank_w[l] : t.rank_p[l]);
        for (uint64_t m = __ballot(path && lo < b && (hi > lo ? hi : lo + 1) > a); m; m &= m - 1) {
            const int j = __ffsll(static_cast<u64>(m)) - 1;
            const uint64_t f_lo = shfl64(lo, j), f_hi = shfl64(hi, j), f_row = shfl64(row, j), f_line = base + j;
            const bool walk = __shfl(static_cast<uint32_t>(kind), j, 64) == KIND_W;
            const uint32_t in_field = range_mask(p0, f_lo, f_hi);
            const uint32_t mine = walk ? marks_w & in_field : (marks_p & in_field) | first_byte_bit(p0, f_lo, f_hi);
            uint32_t total;
            const uint64_t at = (walk ? done_w : done_p) + wave_exclusive(__popc(mine), total);
            if (lane == 0) {
                if (f_lo >= a) step_off[f_row] = walk ? done_w : done_p;
                if (f_hi > f_lo) {
                    // what no token's lane sees: a walk starts with a mark, a list of steps does not end in a ','
                    if (walk && f_lo >= a && text[f_lo] != '>' && text[f_lo] != '<') post(err, f_line, GFA_ERR_NAMED_STEP);
                    if (!walk && f_hi - 1 >= a && f_hi - 1 < b && text[f_hi - 1] != '+' && text[f_hi - 1] != '-') post(err, f_line, GFA_ERR_NAMED_STEP);
                }
            }
            uint32_t k = 0;
            for (uint32_t mm = mine; mm; mm &= mm - 1, k++) {
                const uint64_t q = p0 + (__ffs(mm) - 1);
                uint32_t segment = 0, reverse = 0, step = 0;
                uint64_t nodes = 0;
                const uint32_t code = parse_named_step(text, f_lo, f_hi, q, walk, names, segment, reverse);
                if (code) post(err, f_line, code);
                else {
                    step = 2 * segment + reverse;
                    nodes = seg_start[segment + 1] - seg_start[segment];
                    if (!((visited[segment >> 5] >> (segment & 31)) & 1u)) atomicOr(&visited[segment >> 5], 1u << (segment & 31));
                }
                step_seg[at + k] = step; step_nodes[at + k] = nodes;
            }
            if (walk) done_w += total; else done_p += total;
        }
    }
}

// ---- translated: expand -----------------------------------------------------------------------------------------------------------------

// node_off: the scanned node counts of the steps ([steps + 1]); the row offsets of the paths in nodes
__global__ __launch_bounds__(THREADS) void k_gfa_path_offsets(const uint64_t *__restrict__ step_off, const uint64_t *__restrict__ node_off, uint64_t n_paths, uint64_t *__restrict__ offsets) {
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (p > n_paths) return;
    offsets[p] = node_off[step_off[p]];
}

// One lane per output node: its step by bisection; a forward step is the nodes of its segment ascending, a reverse step descending
__global__ __launch_bounds__(THREADS) void k_gfa_expand_steps(const uint64_t *__restrict__ node_off, const uint32_t *__restrict__ step_seg, uint64_t steps,
                                                              const uint64_t *__restrict__ seg_start, uint64_t total, uint32_t *__restrict__ nodes) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (i >= total) return;
    const uint64_t st = upper_bound(node_off, 0, steps + 1, i) - 1;
    const uint32_t step = step_seg[st], segment = step >> 1, reverse = step & 1u;
    const uint64_t first = seg_start[segment] + 1, count = seg_start[segment + 1] - seg_start[segment], j = i - node_off[st];
    const uint64_t node = reverse ? first + (count - 1 - j) : first + j;
    nodes[i] = static_cast<uint32_t>(2 * node + reverse);
}

// ---- labels ----------------------------------------------------------------------------------------------------------------------------

// ids sorted (stably: the lines of one id stay in file order): the second line of an id is refused
__global__ __launch_bounds__(THREADS) void k_gfa_duplicates(const uint32_t *__restrict__ ids, const uint32_t *__restrict__ segs, const uint32_t *__restrict__ seg_line, uint64_t n, u64 *err) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (i == 0 || i >= n) return;
    if (ids[i] == ids[i - 1]) post(err, seg_line[segs[i]], GFA_ERR_DUPLICATE);
}

// slot = id - min_id of every visited S-line: the length of its label and where it lies in the text
__global__ __launch_bounds__(THREADS) void k_gfa_label_slots(const uint32_t *__restrict__ seg_id, const uint32_t *__restrict__ seg_line, uint64_t n, const uint32_t *__restrict__ visited,
                                                             LineTables t, uint64_t min_id, uint64_t slots, uint64_t *__restrict__ slot_len, uint64_t *__restrict__ slot_src, u64 *counters) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = seg_id[i];
    if (!((visited[id >> 5] >> (id & 31)) & 1u) || id < min_id || id - min_id >= slots) return;
    const uint64_t l = seg_line[i];
    slot_len[id - min_id] = t.hi[l] - t.lo[l];
    slot_src[id - min_id] = t.lo[l];
    atomicAdd(&counters[CNT_GRAPH_NODES], 1ull);
}


// Translated: slot = node - 1 of every node of a visited segment: its chunk of the segment's sequence (all but the last are max_node_length long)
__global__ __launch_bounds__(THREADS) void k_gfa_node_slots(const uint64_t *__restrict__ seg_start, const uint32_t *__restrict__ seg_line, uint64_t segments, const uint32_t *__restrict__ visited,
                                                            LineTables t, uint32_t max_node_length, uint64_t nodes, uint64_t *__restrict__ slot_len, uint64_t *__restrict__ slot_src, u64 *counters) {
    const uint64_t v = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (v >= nodes) return;
    const uint64_t k = upper_bound(seg_start, 0, segments + 1, v) - 1;
    if (!((visited[k >> 5] >> (k & 31)) & 1u)) return;
    const uint64_t l = seg_line[k], bases = t.hi[l] - t.lo[l], from = (v - seg_start[k]) * max_node_length;
    slot_len[v] = max_node_length && bases - from > max_node_length ? max_node_length : bases - from;
    slot_src[v] = t.lo[l] + from;
    atomicAdd(&counters[CNT_GRAPH_NODES], 1ull);
}

// The stored name of a segment: its name if a path visits it, else empty
__global__ __launch_bounds__(THREADS) void k_gfa_name_slots(const uint64_t *__restrict__ name_lo, const uint32_t *__restrict__ name_len, uint64_t segments, const uint32_t *__restrict__ visited,
                                                            uint64_t *__restrict__ slot_len, uint64_t *__restrict__ slot_src) {
    const uint64_t k = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (k >= segments) return;
    const bool seen = (visited[k >> 5] >> (k & 31)) & 1u;
    slot_len[k] = seen ? name_len[k] : 0;
    slot_src[k] = name_lo[k];
}

// 16 output bytes per lane (out is padded to a multiple of 16): the slot of a byte by bisection over the offsets, kept while it lasts
__global__ __launch_bounds__(THREADS) void k_gfa_copy_labels(const uint8_t *__restrict__ text, const uint64_t *__restrict__ slot_off, const uint64_t *__restrict__ slot_src,
                                                             uint64_t slots, uint64_t total, uint8_t *__restrict__ out) {
    const uint64_t first = (static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x) * 16;
    if (first >= total) return;
    uint32_t w[4] = {0, 0, 0, 0};
    uint64_t s = upper_bound(slot_off, 0, slots + 1, first) - 1;
    for (uint32_t i = 0; i < 16 && first + i < total; i++) {
        const uint64_t pos = first + i;
        if (pos >= slot_off[s + 1]) s = upper_bound(slot_off, s + 1, slots + 1, pos) - 1;
        w[i / 4] |= static_cast<uint32_t>(text[slot_src[s] + (pos - slot_off[s])]) << (8 * (i % 4));
    }
    *reinterpret_cast<uint4 *>(out + first) = make_uint4(w[0], w[1], w[2], w[3]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------

using Tally = CountedScratch;
using Buf = CountedBuf;

using Event = EventSet<1>;

// (at least one block: a launch over no items is a launch of idle lanes, not an error)
inline unsigned blocks_or_one(uint64_t items, uint64_t per_block) { return static_cast<unsigned>(std::max<uint64_t>(1, (items + per_block - 1) / per_block)); }

// exclusive_sum in place, with a temp of its own that is gone when it returns
template <class T>
void exclusive_sum(Tally &tally, T *data, uint64_t n, hipStream_t s) {
    Buf temp;
    exclusive_sum(data, data, n, tally, temp, s);
    HIP_CHECK(hipStreamSynchronize(s));       // (temp goes)
}

}  // namespace

struct GfaDeviceParse::Impl {
    hipStream_t s = nullptr;
    uint64_t len = 0, tiles = 0, lines = 0, tabs = 0, max_id = 0;
    Tally tally, rows_tally;      // rows_tally: the rows, which nobody reports
    Buf text, tile_nl, tile_tab, nl_pos, tab_pos, kind, first_tab, lo, hi, id, rank_h, rank_s, rank_p, rank_w, words, seg_id, seg_line, present, visited, tile_p, tile_w;
    Buf offsets, nodes;                       // the rows: the caller's, counted apart (rows_tally)
    // a translated parse
    GfaParseOptions options;
    Buf name_lo, name_len, hash, rank, bucket, seg_start;
    GfaNameTable names{};
    void translated_rows(uint64_t steps_p, Event &e_names0, Event &e_names1, Event &e_expand0, Event &e_expand1, GfaDeviceParse &out);
    LineTables tables{};
    u64 *counters() const { return words.as<u64>(); }
    u64 *err() const { return words.as<u64>() + CNT_WORDS; }
};

GfaDeviceParse::GfaDeviceParse(const char *text, uint64_t len, hipStream_t s, GfaParseOptions options) : impl(new Impl) {
    try {
        Impl &m = *impl;
        m.s = s;
        m.options = options;
        const auto t0 = std::chrono::steady_clock::now();
        const bool add_newline = len != 0 && text[len - 1] != '\n';       // the last line may lack its newline: it gets one here
        m.len = len + (add_newline ? 1 : 0);
        m.tiles = (m.len + GFA_TILE_BYTES - 1) / GFA_TILE_BYTES;
        if (m.tiles >= GFA_MAX_LINES) throw Unsupported("a GFA text of more than 2^41 bytes is not supported");
        counts.bytes = len;
        const size_t padded = static_cast<size_t>(m.tiles) * GFA_TILE_BYTES + GFA_TEXT_PAD;
        m.text.alloc(m.tally, padded);
        if (len) HIP_CHECK(hipMemcpyAsync(m.text.ptr, text, len, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(m.text.as<uint8_t>() + len, 0, padded - len, s));
        if (add_newline) HIP_CHECK(hipMemsetAsync(m.text.as<uint8_t>() + len, '\n', 1, s));
        HIP_CHECK(hipStreamSynchronize(s));
        upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    } catch (...) { delete impl; throw; }
}

GfaDeviceParse::~GfaDeviceParse() { delete impl; }

const uint64_t *GfaDeviceParse::d_offsets() const { return impl->offsets.as<uint64_t>(); }
const uint32_t *GfaDeviceParse::d_nodes() const { return impl->nodes.as<uint32_t>(); }

void GfaDeviceParse::rows() {
    Impl &m = *impl;
    hipStream_t s = m.s;
    const uint8_t *text = m.text.as<uint8_t>();
    Event e0, e1, e2, e_names0, e_names1, e_expand0, e_expand1;
    const bool by_name = m.options.translate != GBWT_HIP_GFA_TRANSLATE_NEVER;
    m.words.alloc(m.tally, (CNT_WORDS + 1) * sizeof(u64));
    HIP_CHECK(hipMemsetAsync(m.words.ptr, 0, CNT_WORDS * sizeof(u64), s));
    HIP_CHECK(hipMemsetAsync(m.err(), 0xFF, sizeof(u64), s));
    m.offsets.alloc(m.rows_tally, sizeof(uint64_t));
    HIP_CHECK(hipMemsetAsync(m.offsets.ptr, 0, sizeof(uint64_t), s));
    HIP_CHECK(hipEventRecord(e0[0], s));
    if (m.tiles == 0) { HIP_CHECK(hipStreamSynchronize(s)); peak_bytes = m.tally.peak; return; }

    // -- structure
    const unsigned tile_blocks = blocks_or_one(m.tiles, WAVES);
    m.tile_nl.alloc(m.tally, (m.tiles + 1) * sizeof(uint64_t));
    m.tile_tab.alloc(m.tally, (m.tiles + 1) * sizeof(uint64_t));
    HIP_CHECK(hipMemsetAsync(m.tile_nl.as<uint64_t>() + m.tiles, 0, sizeof(uint64_t), s));
    HIP_CHECK(hipMemsetAsync(m.tile_tab.as<uint64_t>() + m.tiles, 0, sizeof(uint64_t), s));
    hipLaunchKernelGGL(k_gfa_count_structure, dim3(tile_blocks), dim3(THREADS), 0, s, text, m.tiles, m.tile_nl.as<uint64_t>(), m.tile_tab.as<uint64_t>());
    HIP_CHECK(hipGetLastError());
    exclusive_sum(m.tally, m.tile_nl.as<uint64_t>(), m.tiles + 1, s);       // (the entry behind the last tile: the total)
    exclusive_sum(m.tally, m.tile_tab.as<uint64_t>(), m.tiles + 1, s);
    uint64_t totals[2];
    HIP_CHECK(hipMemcpy(&totals[0], m.tile_nl.as<uint64_t>() + m.tiles, sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(&totals[1], m.tile_tab.as<uint64_t>() + m.tiles, sizeof(uint64_t), hipMemcpyDeviceToHost));
    m.lines = totals[0]; m.tabs = totals[1];
    if (m.lines > GFA_MAX_LINES) throw Unsupported("a GFA text of more than 2^31 - 1 lines is not supported");
    const uint64_t L = m.lines;
    m.nl_pos.alloc(m.tally, L * sizeof(uint64_t));
    m.tab_pos.alloc(m.tally, m.tabs * sizeof(uint64_t));
    hipLaunchKernelGGL(k_gfa_record_structure, dim3(tile_blocks), dim3(THREADS), 0, s, text, m.tiles, m.tile_nl.as<uint64_t>(), m.tile_tab.as<uint64_t>(), m.nl_pos.as<uint64_t>(),
                       m.tab_pos.as<uint64_t>(), m.err());
    HIP_CHECK(hipGetLastError());
    m.tile_tab.release();
    m.kind.alloc(m.tally, L); m.first_tab.alloc(m.tally, L * sizeof(uint64_t)); m.lo.alloc(m.tally, L * sizeof(uint64_t)); m.hi.alloc(m.tally, L * sizeof(uint64_t));
    m.id.alloc(m.tally, L * sizeof(uint32_t));
    for (Buf *r : {&m.rank_h, &m.rank_s, &m.rank_p, &m.rank_w}) r->alloc(m.tally, L * sizeof(uint32_t));
    m.tables = LineTables{m.kind.as<uint8_t>(), m.first_tab.as<uint64_t>(), m.lo.as<uint64_t>(), m.hi.as<uint64_t>(), m.id.as<uint32_t>(),
                          m.rank_h.as<uint32_t>(), m.rank_s.as<uint32_t>(), m.rank_p.as<uint32_t>(), m.rank_w.as<uint32_t>()};
    const unsigned line_blocks = blocks_or_one(L, THREADS);
    hipLaunchKernelGGL(k_gfa_lines, dim3(line_blocks), dim3(THREADS), 0, s, text, m.nl_pos.as<uint64_t>(), L, m.tab_pos.as<uint64_t>(), m.tabs, m.tables, by_name ? 1u : 0u, m.counters(), m.err());
    HIP_CHECK(hipGetLastError());
    for (Buf *r : {&m.rank_h, &m.rank_s, &m.rank_p, &m.rank_w}) exclusive_sum(m.tally, r->as<uint32_t>(), L, s);
    u64 c[CNT_WORDS];
    HIP_CHECK(hipMemcpy(c, m.counters(), sizeof(c), hipMemcpyDeviceToHost));
    counts.lines = c[CNT_LINES]; counts.headers = c[CNT_H]; counts.segments = c[CNT_S]; counts.links = c[CNT_L]; counts.p_lines = c[CNT_P]; counts.w_lines = c[CNT_W];
    counts.ignored_lines = c[CNT_IGNORED]; counts.label_bytes = c[CNT_LABEL_BYTES];
    m.max_id = c[CNT_MAX_ID];
    // AUTO: a name that is no node id, or a sequence to chop.  A text without segments has nothing to translate.
    translated = counts.segments != 0 && (m.options.translate == GBWT_HIP_GFA_TRANSLATE_ALWAYS ||
                                          (by_name && (c[CNT_NOT_ID] != 0 || (m.options.max_node_length != 0 && c[CNT_MAX_SEQUENCE] > m.options.max_node_length))));
    n_paths = counts.p_lines + counts.w_lines;
    Buf headers, paths;
    headers.alloc(m.tally, 2 * counts.headers * sizeof(uint64_t));
    paths.alloc(m.tally, n_paths * sizeof(GfaPathLine));
    m.seg_id.alloc(m.tally, counts.segments * sizeof(uint32_t)); m.seg_line.alloc(m.tally, counts.segments * sizeof(uint32_t));
    const size_t bit_words = static_cast<size_t>((translated ? counts.segments : m.max_id) / 32 + 1);     // translated: a bit per segment, and no table over the ids
    if (!translated) m.present.alloc(m.tally, bit_words * sizeof(uint32_t));
    m.visited.alloc(m.tally, bit_words * sizeof(uint32_t));
    if (!translated) HIP_CHECK(hipMemsetAsync(m.present.ptr, 0, bit_words * sizeof(uint32_t), s));
    HIP_CHECK(hipMemsetAsync(m.visited.ptr, 0, bit_words * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_gfa_gather_lines, dim3(line_blocks), dim3(THREADS), 0, s, m.nl_pos.as<uint64_t>(), L, m.tab_pos.as<uint64_t>(), m.tables, counts.p_lines,
                       headers.as<uint64_t>(), m.seg_id.as<uint32_t>(), m.seg_line.as<uint32_t>(), m.present.as<uint32_t>(), paths.as<GfaPathLine>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(e1[0], s));
    path_lines.resize(n_paths);
    if (n_paths) HIP_CHECK(hipMemcpyAsync(path_lines.data(), paths.ptr, n_paths * sizeof(GfaPathLine), hipMemcpyDeviceToHost, s));
    std::vector<uint64_t> h(2 * counts.headers);
    if (!h.empty()) HIP_CHECK(hipMemcpyAsync(h.data(), headers.ptr, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));

    // -- steps
    m.tile_p.alloc(m.tally, (m.tiles + 1) * sizeof(uint64_t)); m.tile_w.alloc(m.tally, (m.tiles + 1) * sizeof(uint64_t));
    HIP_CHECK(hipMemsetAsync(m.tile_p.as<uint64_t>() + m.tiles, 0, sizeof(uint64_t), s));
    HIP_CHECK(hipMemsetAsync(m.tile_w.as<uint64_t>() + m.tiles, 0, sizeof(uint64_t), s));
    if (translated) hipLaunchKernelGGL(k_gfa_count_tokens, dim3(tile_blocks), dim3(THREADS), 0, s, text, m.tiles, m.tile_nl.as<uint64_t>(), L, m.tables, m.tile_p.as<uint64_t>(), m.tile_w.as<uint64_t>());
    else hipLaunchKernelGGL(k_gfa_count_steps, dim3(tile_blocks), dim3(THREADS), 0, s, text, m.tiles, m.tile_nl.as<uint64_t>(), L, m.tables, m.tile_p.as<uint64_t>(), m.tile_w.as<uint64_t>());
    HIP_CHECK(hipGetLastError());
    exclusive_sum(m.tally, m.tile_p.as<uint64_t>(), m.tiles + 1, s);
    exclusive_sum(m.tally, m.tile_w.as<uint64_t>(), m.tiles + 1, s);
    uint64_t steps_p = 0, steps_w = 0;
    HIP_CHECK(hipMemcpy(&steps_p, m.tile_p.as<uint64_t>() + m.tiles, sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(&steps_w, m.tile_w.as<uint64_t>() + m.tiles, sizeof(uint64_t), hipMemcpyDeviceToHost));
    counts.steps = steps_p + steps_w;
    for (size_t k = 0; k < counts.headers; k++) header_lines.emplace_back(h[2 * k], h[2 * k + 1]);
    headers.release(); paths.release();
    row_nodes = counts.steps;
    if (translated) {
        m.translated_rows(steps_p, e_names0, e_names1, e_expand0, e_expand1, *this);
    } else {
        m.offsets.alloc(m.rows_tally, (n_paths + 1) * sizeof(uint64_t));
        m.nodes.alloc(m.rows_tally, counts.steps * sizeof(uint32_t));
        HIP_CHECK(hipMemcpyAsync(m.offsets.as<uint64_t>() + n_paths, &counts.steps, sizeof(uint64_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_gfa_fill_steps, dim3(tile_blocks), dim3(THREADS), 0, s, text, m.tiles, m.tile_nl.as<uint64_t>(), L, m.tables, m.tile_p.as<uint64_t>(), m.tile_w.as<uint64_t>(),
                           counts.p_lines, steps_p, m.present.as<uint32_t>(), m.max_id, m.visited.as<uint32_t>(), m.offsets.as<uint64_t>(), m.nodes.as<uint32_t>(), m.err());
        HIP_CHECK(hipGetLastError());

        // -- duplicates of an S id (they would make the label of a node ambiguous; found here so that the refusal is complete before the rows are used)
        const uint64_t S = counts.segments;
        if (S > 1) {
            Buf keys, vals_in, vals, temp;
            keys.alloc(m.tally, S * sizeof(uint32_t)); vals_in.alloc(m.tally, S * sizeof(uint32_t)); vals.alloc(m.tally, S * sizeof(uint32_t));
            std::vector<uint32_t> iota(S);
            for (uint64_t i = 0; i < S; i++) iota[i] = static_cast<uint32_t>(i);
            HIP_CHECK(hipMemcpyAsync(vals_in.ptr, iota.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            size_t bytes = 0;
            HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, m.seg_id.as<uint32_t>(), keys.as<uint32_t>(), vals_in.as<uint32_t>(), vals.as<uint32_t>(), static_cast<int>(S), 0, 31, s));
            temp.alloc(m.tally, bytes);
            HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp.ptr, bytes, m.seg_id.as<uint32_t>(), keys.as<uint32_t>(), vals_in.as<uint32_t>(), vals.as<uint32_t>(), static_cast<int>(S), 0, 31, s));
            hipLaunchKernelGGL(k_gfa_duplicates, dim3(blocks_or_one(S, THREADS)), dim3(THREADS), 0, s, keys.as<uint32_t>(), vals.as<uint32_t>(), m.seg_line.as<uint32_t>(), S, m.err());
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipStreamSynchronize(s));
        }
    }
    HIP_CHECK(hipEventRecord(e2[0], s));
    u64 word = 0;
    HIP_CHECK(hipMemcpyAsync(&word, m.err(), sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipEventElapsedTime(&structure_ms, e0[0], e1[0]));
    HIP_CHECK(hipEventElapsedTime(&steps_ms, e1[0], e2[0]));
    if (word != ~u64(0)) { refusal.line = (word >> 8) + 1; refusal.code = static_cast<uint32_t>(word & 0xFF); }
    else if (translated) {
        // the alphabet is all the nodes, visited or not: the mapping of a GBZ has one slot per potential node
        min_node = 2; max_node = static_cast<uint32_t>(2 * total_nodes + 1);
        HIP_CHECK(hipEventElapsedTime(&names_ms, e_names0[0], e_names1[0]));
        HIP_CHECK(hipEventElapsedTime(&expand_ms, e_expand0[0], e_expand1[0]));
    } else if (counts.steps) build_node_range(m.nodes.as<uint32_t>(), counts.steps, min_node, max_node, s);
    // what only the steps needed
    m.tile_nl.release(); m.tile_p.release(); m.tile_w.release(); m.nl_pos.release(); m.tab_pos.release(); m.first_tab.release(); m.present.release();
    m.rank_h.release(); m.rank_s.release(); m.rank_p.release(); m.rank_w.release(); m.id.release(); m.kind.release();
    peak_bytes = m.tally.peak;
}


// The steps of a translated parse, from the token counts of the tiles (tile_p / tile_w: scanned) to the rows.  After a refusal the rows
// are not expanded.
void GfaDeviceParse::Impl::translated_rows(uint64_t steps_p, Event &e_names0, Event &e_names1, Event &e_expand0, Event &e_expand1, GfaDeviceParse &out) {
    Impl &m = *this;
    const uint8_t *txt = m.text.as<uint8_t>();
    const uint64_t S = out.counts.segments, T = out.counts.steps, n_paths = out.n_paths, L = m.lines;
    const unsigned tile_blocks = blocks_or_one(m.tiles, WAVES);
    if (T + 1 > GFA_MAX_LINES) throw Unsupported("more than 2^31 - 2 steps are not supported");

    // -- names: the plan of the segments and the table of their names
    HIP_CHECK(hipEventRecord(e_names0[0], s));
    const uint32_t bits = gfa_bucket_bits(S);
    const uint64_t buckets = (uint64_t(1) << bits) + 1;
    Buf hash_in, rank_in;
    m.name_lo.alloc(m.tally, S * sizeof(uint64_t)); m.name_len.alloc(m.tally, S * sizeof(uint32_t));
    hash_in.alloc(m.tally, S * sizeof(uint64_t)); rank_in.alloc(m.tally, S * sizeof(uint32_t));
    m.hash.alloc(m.tally, S * sizeof(uint64_t)); m.rank.alloc(m.tally, S * sizeof(uint32_t));
    m.bucket.alloc(m.tally, buckets * sizeof(uint32_t));
    m.seg_start.alloc(m.tally, (S + 1) * sizeof(uint64_t));
    HIP_CHECK(hipMemsetAsync(m.seg_start.as<uint64_t>() + S, 0, sizeof(uint64_t), s));
    hipLaunchKernelGGL(k_gfa_segment_plan, dim3(blocks_or_one(S, THREADS)), dim3(THREADS), 0, s, txt, m.tab_pos.as<uint64_t>(), m.tables, m.seg_line.as<uint32_t>(), S, m.options.max_node_length,
                       m.name_lo.as<uint64_t>(), m.name_len.as<uint32_t>(), hash_in.as<uint64_t>(), rank_in.as<uint32_t>(), m.seg_start.as<uint64_t>(), m.counters());
    HIP_CHECK(hipGetLastError());
    exclusive_sum(m.tally, m.seg_start.as<uint64_t>(), S + 1, s);
    HIP_CHECK(hipMemcpy(&out.total_nodes, m.seg_start.as<uint64_t>() + S, sizeof(uint64_t), hipMemcpyDeviceToHost));
    {
        Buf temp;
        size_t bytes = 0;
        HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, hash_in.as<uint64_t>(), m.hash.as<uint64_t>(), rank_in.as<uint32_t>(), m.rank.as<uint32_t>(), static_cast<int>(S), 0, 64, s));
        temp.alloc(m.tally, bytes);
        HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp.ptr, bytes, hash_in.as<uint64_t>(), m.hash.as<uint64_t>(), rank_in.as<uint32_t>(), m.rank.as<uint32_t>(), static_cast<int>(S), 0, 64, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    hash_in.release(); rank_in.release();
    m.names = GfaNameTable{txt, m.name_lo.as<uint64_t>(), m.name_len.as<uint32_t>(), m.hash.as<uint64_t>(), m.rank.as<uint32_t>(), m.bucket.as<uint32_t>(), bits, static_cast<uint32_t>(S)};
    hipLaunchKernelGGL(k_gfa_name_duplicates, dim3(blocks_or_one(S, THREADS)), dim3(THREADS), 0, s, m.names, m.seg_line.as<uint32_t>(), m.err());
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_gfa_name_buckets, dim3(blocks_or_one(buckets, THREADS)), dim3(THREADS), 0, s, m.hash.as<uint64_t>(), S, bits, m.bucket.as<uint32_t>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(e_names1[0], s));
    out.table_bytes = S * (2 * sizeof(uint64_t) + 2 * sizeof(uint32_t)) + buckets * sizeof(uint32_t);

    // -- steps: (segment, orientation) and the node count of every token
    Buf step_off, step_seg, node_off;
    step_off.alloc(m.tally, (n_paths + 1) * sizeof(uint64_t));
    step_seg.alloc(m.tally, T * sizeof(uint32_t));
    node_off.alloc(m.tally, (T + 1) * sizeof(uint64_t));
    HIP_CHECK(hipMemcpyAsync(step_off.as<uint64_t>() + n_paths, &T, sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(node_off.as<uint64_t>() + T, 0, sizeof(uint64_t), s));
    hipLaunchKernelGGL(k_gfa_fill_tokens, dim3(tile_blocks), dim3(THREADS), 0, s, txt, m.tiles, m.tile_nl.as<uint64_t>(), L, m.tables, m.tile_p.as<uint64_t>(), m.tile_w.as<uint64_t>(),
                       out.counts.p_lines, steps_p, m.names, m.seg_start.as<uint64_t>(), m.visited.as<uint32_t>(), step_off.as<uint64_t>(), step_seg.as<uint32_t>(), node_off.as<uint64_t>(),
                       m.err());
    HIP_CHECK(hipGetLastError());
    u64 word = 0, chopped = 0;
    HIP_CHECK(hipMemcpyAsync(&word, m.err(), sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&chopped, m.counters() + CNT_CHOPPED, sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    out.chopped_segments = chopped;

    // -- expand: every step becomes the nodes of its segment
    HIP_CHECK(hipEventRecord(e_expand0[0], s));
    out.row_nodes = 0;
    m.offsets.alloc(m.rows_tally, (n_paths + 1) * sizeof(uint64_t));
    if (word == ~u64(0)) {
        if (out.total_nodes > 0x7FFFFFFFull) throw Unsupported(std::to_string(out.total_nodes) + " nodes after chopping: more than 2^31 - 1 are not supported");
        exclusive_sum(m.tally, node_off.as<uint64_t>(), T + 1, s);
        HIP_CHECK(hipMemcpy(&out.row_nodes, node_off.as<uint64_t>() + T, sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (out.row_nodes > BUILD_MAX_SLOTS) throw Unsupported(std::to_string(out.row_nodes) + " visits: more than 2^32 - 1 are not supported (u32 positions on device)");
        m.nodes.alloc(m.rows_tally, out.row_nodes * sizeof(uint32_t));
        hipLaunchKernelGGL(k_gfa_path_offsets, dim3(blocks_or_one(n_paths + 1, THREADS)), dim3(THREADS), 0, s, step_off.as<uint64_t>(), node_off.as<uint64_t>(), n_paths, m.offsets.as<uint64_t>());
        HIP_CHECK(hipGetLastError());
        if (out.row_nodes) {
            hipLaunchKernelGGL(k_gfa_expand_steps, dim3(blocks_or_one(out.row_nodes, THREADS)), dim3(THREADS), 0, s, node_off.as<uint64_t>(), step_seg.as<uint32_t>(), T, m.seg_start.as<uint64_t>(),
                               out.row_nodes, m.nodes.as<uint32_t>());
            HIP_CHECK(hipGetLastError());
        }
    }
    HIP_CHECK(hipEventRecord(e_expand1[0], s));
    HIP_CHECK(hipStreamSynchronize(s));        // (step_off, step_seg and node_off go)
    m.hash.release(); m.rank.release(); m.bucket.release();
}

void GfaDeviceParse::labels(Strings &out, uint64_t &graph_nodes) {
    Impl &m = *impl;
    hipStream_t s = m.s;
    out = Strings();
    graph_nodes = 0;
    if (row_nodes == 0) return;
    const uint64_t min_id = min_node / 2, slots = max_node / 2 - min_id + 1, S = counts.segments;       // (translated: nodes 1 .. total_nodes)
    Event e0, e1;
    HIP_CHECK(hipEventRecord(e0[0], s));
    Buf slot_off, slot_src, bytes;
    slot_off.alloc(m.tally, (slots + 1) * sizeof(uint64_t)); slot_src.alloc(m.tally, slots * sizeof(uint64_t));
    HIP_CHECK(hipMemsetAsync(slot_off.ptr, 0, (slots + 1) * sizeof(uint64_t), s));
    HIP_CHECK(hipMemsetAsync(slot_src.ptr, 0, slots * sizeof(uint64_t), s));
    if (translated)
        hipLaunchKernelGGL(k_gfa_node_slots, dim3(blocks_or_one(slots, THREADS)), dim3(THREADS), 0, s, m.seg_start.as<uint64_t>(), m.seg_line.as<uint32_t>(), S, m.visited.as<uint32_t>(), m.tables,
                           m.options.max_node_length, slots, slot_off.as<uint64_t>(), slot_src.as<uint64_t>(), m.counters());
    else
        hipLaunchKernelGGL(k_gfa_label_slots, dim3(blocks_or_one(S, THREADS)), dim3(THREADS), 0, s, m.seg_id.as<uint32_t>(), m.seg_line.as<uint32_t>(), S, m.visited.as<uint32_t>(), m.tables,
                           min_id, slots, slot_off.as<uint64_t>(), slot_src.as<uint64_t>(), m.counters());
    HIP_CHECK(hipGetLastError());
    exclusive_sum(m.tally, slot_off.as<uint64_t>(), slots + 1, s);
    uint64_t total = 0;
    HIP_CHECK(hipMemcpy(&total, slot_off.as<uint64_t>() + slots, sizeof(uint64_t), hipMemcpyDeviceToHost));
    const size_t padded = (static_cast<size_t>(total) + 15) / 16 * 16;
    bytes.alloc(m.tally, padded);
    if (total) {
        hipLaunchKernelGGL(k_gfa_copy_labels, dim3(blocks_or_one(padded / 16, THREADS)), dim3(THREADS), 0, s, m.text.as<uint8_t>(), slot_off.as<uint64_t>(), slot_src.as<uint64_t>(), slots, total,
                           bytes.as<uint8_t>());
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(e1[0], s));
    out.offsets.resize(slots + 1);
    out.bytes.resize(total);
    HIP_CHECK(hipMemcpyAsync(out.offsets.data(), slot_off.ptr, (slots + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (total) HIP_CHECK(hipMemcpyAsync(out.bytes.data(), bytes.ptr, total, hipMemcpyDeviceToHost, s));
    u64 nodes = 0;
    HIP_CHECK(hipMemcpyAsync(&nodes, m.counters() + CNT_GRAPH_NODES, sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipEventElapsedTime(&labels_ms, e0[0], e1[0]));
    graph_nodes = nodes;
    peak_bytes = m.tally.peak;
}

void GfaDeviceParse::translation(GfaTranslation &out) {
    Impl &m = *impl;
    hipStream_t s = m.s;
    out = GfaTranslation();
    if (!translated || row_nodes == 0) return;
    const uint64_t S = counts.segments;
    Buf slot_off, slot_src, bytes;
    slot_off.alloc(m.tally, (S + 1) * sizeof(uint64_t)); slot_src.alloc(m.tally, S * sizeof(uint64_t));
    HIP_CHECK(hipMemsetAsync(slot_off.as<uint64_t>() + S, 0, sizeof(uint64_t), s));
    hipLaunchKernelGGL(k_gfa_name_slots, dim3(blocks_or_one(S, THREADS)), dim3(THREADS), 0, s, m.name_lo.as<uint64_t>(), m.name_len.as<uint32_t>(), S, m.visited.as<uint32_t>(),
                       slot_off.as<uint64_t>(), slot_src.as<uint64_t>());
    HIP_CHECK(hipGetLastError());
    exclusive_sum(m.tally, slot_off.as<uint64_t>(), S + 1, s);
    uint64_t total = 0;
    HIP_CHECK(hipMemcpy(&total, slot_off.as<uint64_t>() + S, sizeof(uint64_t), hipMemcpyDeviceToHost));
    const size_t padded = (static_cast<size_t>(total) + 15) / 16 * 16;
    bytes.alloc(m.tally, padded);
    if (total) {
        hipLaunchKernelGGL(k_gfa_copy_labels, dim3(blocks_or_one(padded / 16, THREADS)), dim3(THREADS), 0, s, m.text.as<uint8_t>(), slot_off.as<uint64_t>(), slot_src.as<uint64_t>(), S, total,
                           bytes.as<uint8_t>());
        HIP_CHECK(hipGetLastError());
    }
    out.names.offsets.resize(S + 1);
    out.names.bytes.resize(total);
    out.starts.resize(S);
    HIP_CHECK(hipMemcpyAsync(out.names.offsets.data(), slot_off.ptr, (S + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (total) HIP_CHECK(hipMemcpyAsync(out.names.bytes.data(), bytes.ptr, total, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(out.starts.data(), m.seg_start.ptr, S * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (uint64_t k = 0; k < S; k++) {
        out.starts[k] += 1;                    // the first segment starts at node 1
        unvisited_segments += out.names.offsets[k + 1] == out.names.offsets[k];
    }
    out.mapping_len = total_nodes + 1;
    name_bytes = total;
    peak_bytes = m.tally.peak;
}

void GfaDeviceParse::release_all_but_rows() {
    Impl &m = *impl;
    for (Buf *b : {&m.text, &m.tile_nl, &m.tile_tab, &m.nl_pos, &m.tab_pos, &m.kind, &m.first_tab, &m.lo, &m.hi, &m.id, &m.rank_h, &m.rank_s, &m.rank_p, &m.rank_w, &m.words, &m.seg_id,
                   &m.seg_line, &m.present, &m.visited, &m.tile_p, &m.tile_w, &m.name_lo, &m.name_len, &m.hash, &m.rank, &m.bucket, &m.seg_start})
        b->release();
}

}  // namespace gbwt_hip
