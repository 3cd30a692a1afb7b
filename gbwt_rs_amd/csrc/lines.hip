// lines.hip -- the kernels that turn extracted rows into the P- and W-lines of gbunzip's GFA text (src/bin/gbunzip.rs:456-550), and
// GBZ::segment_path as data.  Launch wrappers declared in lines.hpp; the requests that use them are in capi_lines.hip.
//
// A row is cut into chunks of LINE_CHUNK positions.  Sizing: a wave per chunk sums the bytes of its tokens (">123" / "<123" for walks,
// "123+" / "123-" joined by commas for paths) and its label lengths, scans over the chunks give every line its length -- the header comes
// from the per-path tables built at open, the W-line's end coordinate from the summed label lengths -- or the line cache of the index
// gives it without reading a node id.  Formatting: a workgroup per chunk writes the header (first chunk), the tokens and the trailer (last).
//
// Graphs with a node-to-segment translation (Graph::has_translation, src/graph.rs:158-160) print segment names: SegmentPathIter
// (src/gbz.rs:1098-1169) turns the node sequence into one token per segment.  A path that is a concatenation of whole segments -- every
// path of a GBZ built from a GFA -- is recognised and formatted here (a position is a token iff it is the first node of its segment in the
// orientation of travel, and every other position must continue its predecessor).  A path that is not is flagged and left to the host.
#include "lines.hpp"
#include "scan.hpp"

#include <hipcub/hipcub.hpp>

#include "gfa_tokens.hpp"

namespace gbwt_hip {

namespace {

constexpr int WAVE = 64;
constexpr int FORMAT_THREADS = 256;

__device__ __forceinline__ uint32_t decimal_digits(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}

__device__ __forceinline__ uint32_t decimal_digits64(uint64_t v) {
    uint32_t d = 1;
    while (v >= 10u) { v /= 10u; d++; }
    return d;
}

__global__ void __launch_bounds__(256) k_chunk_counts(const uint64_t *offsets, uint64_t n, uint64_t *counts) {
    const uint64_t p = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (p >= n) return;
    const uint64_t len = offsets[p + 1] - offsets[p];
    counts[p] = len == 0 ? 1 : (len + LINE_CHUNK - 1) / LINE_CHUNK;
}

struct ChunkRange { uint64_t path, begin, lo, hi; bool first, last; };

__device__ __forceinline__ uint64_t chunk_path_of(const uint64_t *chunk_first, uint64_t n, uint64_t c) {
    uint64_t lo = 0, hi = n;                                        // chunk_first[lo] <= c < chunk_first[hi]
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (chunk_first[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// The path of every chunk, once per request: every workgroup (wave) of the kernels below started with this search -- fifteen dependent
// loads for 32 000 paths -- and now starts with one load (round 4: 3 % of config 4's formatting time; with the node ids of a batch asked
// for one batch ahead, 10 %: profiles/r04_gfa_pmc.txt).
__global__ void __launch_bounds__(256) k_chunk_paths(const uint64_t *chunk_first, uint64_t n, uint64_t chunks_cap, uint32_t *chunk_path) {
    const uint64_t c = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (c < chunks_cap && c < chunk_first[n]) chunk_path[c] = static_cast<uint32_t>(chunk_path_of(chunk_first, n, c));
}

__device__ __forceinline__ ChunkRange chunk_range(const uint64_t *chunk_first, const uint32_t *chunk_path, const uint64_t *offsets, uint64_t c) {
    const uint64_t lo = chunk_path[c];
    ChunkRange r;
    r.path = lo;
    r.begin = offsets[lo];
    const uint64_t end = offsets[lo + 1];
    r.lo = r.begin + (c - chunk_first[lo]) * LINE_CHUNK;
    r.hi = r.lo + LINE_CHUNK < end ? r.lo + LINE_CHUNK : end;
    r.first = c == chunk_first[lo];
    r.last = c + 1 == chunk_first[lo + 1];
    return r;
}

// One wave per chunk: text bytes of its node tokens and the summed label lengths (W-line end coordinate,
// src/bin/gbunzip.rs:532-536: sequence_len(node).unwrap_or(0)).
// The number of chunks of a request is known on the device only (chunk_first[n]); the host launches for its upper bound
// (total / LINE_CHUNK + n) and the chunks past the end count nothing, so that the scans over the bound are those over the chunks.
__global__ void __launch_bounds__(256) k_chunk_stats(const uint64_t *offsets, const uint32_t *nodes, uint64_t n, const uint64_t *chunk_first, const uint32_t *chunk_path, uint64_t chunks_cap,
                                                      const uint32_t *label_len, uint64_t n_labels, uint32_t first_node, int p_lines, uint64_t *chunk_text,
                                                      uint64_t *chunk_seq) {
    const uint64_t c = blockIdx.x * static_cast<uint64_t>(blockDim.x / WAVE) + threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    if (c >= chunks_cap) return;
    if (c >= chunk_first[n]) { if (lane == 0) { chunk_text[c] = 0; chunk_seq[c] = 0; } return; }
    const ChunkRange r = chunk_range(chunk_first, chunk_path, offsets, c);
    uint64_t text = 0, labels = 0;
    for (uint64_t k0 = r.lo + 4 * lane; k0 < r.hi; k0 += 4 * WAVE) {   // four consecutive positions per lane: the loads and the label gathers of a round overlap
        uint32_t node[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) node[i] = k0 + i < r.hi ? nodes[k0 + i] : 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            if (k0 + i >= r.hi) continue;
            text += decimal_digits(node[i] >> 1) + 1 + ((p_lines && k0 + i > r.begin) ? 1 : 0);
            const uint64_t seq = (static_cast<uint64_t>(node[i] & ~1u) - first_node) / 2;   // GBZ::graph_node_to_sequence, src/gbz.rs:246-255
            if ((node[i] & ~1u) >= first_node && seq < n_labels) labels += label_len[seq];
        }
    }
    for (int d = WAVE / 2; d > 0; d >>= 1) { text += __shfl_down(text, d, WAVE); labels += __shfl_down(labels, d, WAVE); }
    if (lane == 0) { chunk_text[c] = text; chunk_seq[c] = labels; }
}

// Per path, from the scans over the chunks: the length of its line -- header (prefix from the table + for W-lines the end coordinate and
// its tab), node tokens, trailer -- the end coordinate itself, and for translation graphs whether every position fitted a whole segment
// (bad_before = scan of the chunks' bad flags, or null).  A flagged line gets length 0 here: the host replays it and puts its length in.
__global__ void __launch_bounds__(256) k_line_sizes(const uint64_t *seq_ids, const uint64_t *chunk_first, uint64_t n, const uint64_t *text_before,
                                                     const uint64_t *seq_before, const uint64_t *bad_before, LineHeaders hdr, int p_lines, uint64_t *line_len,
                                                     uint64_t *line_end, uint8_t *valid) {
    const uint64_t p = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (p >= n) return;
    const uint64_t a = chunk_first[p], b = chunk_first[p + 1];
    const uint64_t text = text_before[b] - text_before[a], labels = seq_before[b] - seq_before[a];
    const uint64_t path = seq_ids[p] >> 1;                              // the forward sequence of path p is sequence 2p (support::encode_path)
    uint64_t header = hdr.prefix_off[path + 1] - hdr.prefix_off[path], end = 0;
    if (hdr.fragment) { end = hdr.fragment[path] + labels; header += decimal_digits64(end) + 1; }
    const bool ok = bad_before == nullptr || bad_before[b] == bad_before[a];
    line_end[p] = end;
    line_len[p] = ok ? header + text + (p_lines ? 3u : 1u) : 0u;        // "\t*\n" / "\n"
    if (valid) valid[p] = ok ? 1 : 0;
}

__host__ __device__ __forceinline__ uint64_t cache_p_extra(uint64_t k_chunk) { return k_chunk == 0 ? 0 : k_chunk * LINE_CHUNK - 1; }

// Line lengths and end coordinates from the cache: no node id is read.
__global__ void __launch_bounds__(256) k_line_sizes_cached(const uint64_t *offsets, const uint64_t *seq_ids, uint64_t n, LineCache cache, LineHeaders hdr, int p_lines,
                                                            uint64_t *line_len, uint64_t *line_end) {
    const uint64_t p = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (p >= n) return;
    const uint64_t path = seq_ids[p] >> 1, len = offsets[p + 1] - offsets[p];
    const uint64_t text = cache.path[2 * path] + (p_lines && len != 0 ? len - 1 : 0), labels = cache.path[2 * path + 1];
    uint64_t header = hdr.prefix_off[path + 1] - hdr.prefix_off[path], end = 0;
    if (hdr.fragment) { end = hdr.fragment[path] + labels; header += decimal_digits64(end) + 1; }
    line_end[p] = end;
    line_len[p] = header + text + (p_lines ? 3u : 1u);
}

// The header of a line, written by the workgroup of its first chunk; every chunk needs its length.
__device__ __forceinline__ uint64_t line_header(const LineHeaders &hdr, uint64_t path, const uint64_t *line_end, uint64_t row, bool write, uint8_t *line, uint32_t t,
                                                uint32_t threads) {
    const uint64_t h0 = hdr.prefix_off[path], plen = hdr.prefix_off[path + 1] - h0;
    if (write) for (uint64_t k = t; k < plen; k += threads) line[k] = hdr.prefix[h0 + k];
    if (hdr.fragment == nullptr) return plen;
    uint64_t end = line_end[row];
    const uint32_t digits = decimal_digits64(end);
    if (write && t == 0) {
        for (uint32_t d = 0; d < digits; d++) { line[plen + digits - 1 - d] = static_cast<uint8_t>('0' + end % 10u); end /= 10u; }
        line[plen + digits] = '\t';
    }
    return plen + digits + 1;
}

__global__ void __launch_bounds__(256) k_plan_chunks(const uint64_t *offsets, uint64_t n, const uint64_t *chunk_first, const uint32_t *chunk_path, uint64_t chunks_cap,
                                                      const uint64_t *text_before, int p_lines, const uint64_t *line_start, const uint64_t *seq_ids, LineHeaders hdr,
                                                      const uint64_t *line_end, LineCache cache, ChunkPlan *plans) {
    const uint64_t c = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (c >= chunks_cap || c >= chunk_first[n]) return;
    const ChunkRange r = chunk_range(chunk_first, chunk_path, offsets, c);
    const uint64_t path = seq_ids[r.path] >> 1;
    const uint64_t header_len = line_header(hdr, path, line_end, r.path, false, nullptr, 0, 1);
    // where the chunk's tokens start inside the line: from the scan of this request's sizing pass, or from the line cache of the index
    const uint64_t k_chunk = c - chunk_first[r.path];
    const uint64_t before = cache.text ? cache.text[cache.chunk_first[path] + k_chunk] + (p_lines ? cache_p_extra(k_chunk) : 0) : text_before[c] - text_before[chunk_first[r.path]];
    ChunkPlan plan;
    plan.ids_at = r.lo;
    plan.text_at = line_start[r.path] + header_len + before;
    plan.count = static_cast<uint32_t>(r.hi - r.lo);
    plan.row = static_cast<uint32_t>(r.path);
    plan.flags = (r.first ? 1u : 0u) | (r.last ? 2u : 0u);
    plan.header_len = static_cast<uint32_t>(header_len);
    plans[c] = plan;
}

// One workgroup per chunk: the header (first chunk of a line), the node tokens of the chunk, the trailer (last chunk).
// The tokens of 1 024 positions are put together in LDS (a block scan of their widths places them) and leave as aligned 16-byte
// stores; only the first and the last bytes of such a batch, where the text does not fill a 16-byte unit, go out one by one.
// (With every lane storing its own six bytes one at a time the formatter wrote 330 GB/s of text.)
constexpr uint32_t TOKEN_MAX = 12;   // ',' + ten digits + '+' (P-lines); '>' + ten digits (W-lines)
// PER_THREAD: consecutive positions per thread and batch (one scan and two barriers per 256 * PER_THREAD positions)
// A token is put together in registers (gfa_tokens.hpp) and OR-ed into the staging buffer as the three or four aligned dwords it covers -- the
// buffer is zero wherever no token has been placed, and whoever copies a unit out leaves it zero again.  (Rounds 1-4 made a token with a
// division and a one-byte store per character; that form was bound by exactly those -- vector ALU 83 % busy, LDS 70 %,
// profiles/r05_format_stream.txt -- and lived on behind GBWT_HIP_FORMAT_TOKENS=0 until round 6.)
template <uint32_t PER_THREAD>
__global__ void __launch_bounds__(FORMAT_THREADS) k_format_chunks(const uint32_t *nodes, uint64_t n, const uint64_t *chunk_first, const ChunkPlan *plans, int p_lines,
                                                                   const uint64_t *seq_ids, LineHeaders hdr, const uint64_t *line_end, uint8_t *out) {
    using BlockScan = hipcub::BlockScan<uint32_t, FORMAT_THREADS, hipcub::BLOCK_SCAN_WARP_SCANS>;
    __shared__ typename BlockScan::TempStorage scan_storage;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr uint32_t BATCH = FORMAT_THREADS * PER_THREAD;
    constexpr uint32_t STAGE_BYTES = FORMAT_THREADS * PER_THREAD * TOKEN_MAX + 48;   // a batch, the bytes in front of it in its first unit, the dwords a last token spreads over
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
    if (blockIdx.x >= chunk_first[n]) return;                           // (launched for the host's upper bound of the chunk count)
    const uint32_t t = threadIdx.x;
    const ChunkPlan plan = plans[blockIdx.x];
    uint8_t *const text = out + plan.text_at;
    if (plan.flags & 1u) line_header(hdr, seq_ids[plan.row] >> 1, line_end, plan.row, true, text - plan.header_len, t, FORMAT_THREADS);
    uint64_t cursor = 0;                                                // bytes of the chunk's text written so far
    // positions counted from the start of the chunk (32-bit arithmetic in the loop): `count` of them, the path's first one at `first_at` or nowhere
    const uint32_t count = plan.count, first_at = (plan.flags & 1u) ? 0u : ~0u;
    const uint32_t *const ids = nodes + plan.ids_at;
    uint32_t ahead[PER_THREAD];                                        // the node ids of the next batch are asked for before this one is put together
#pragma unroll
    for (uint32_t i = 0; i < PER_THREAD; i++) { const uint32_t k = PER_THREAD * t + i; ahead[i] = k < count ? ids[k] : 0u; }
    for (uint32_t lo = 16 * t; lo < STAGE_BYTES; lo += 16 * FORMAT_THREADS) *reinterpret_cast<u32x4 *>(stage + lo) = u32x4{0u, 0u, 0u, 0u};   // (while the first node ids are on their way)
    __syncthreads();
    for (uint32_t base = 0; base < count; base += BATCH) {
        const uint32_t k0 = base + PER_THREAD * t;
        uint32_t node[PER_THREAD], digits[PER_THREAD], len = 0;
        Token token[PER_THREAD];
#pragma unroll
        for (uint32_t i = 0; i < PER_THREAD; i++) {
            node[i] = ahead[i]; digits[i] = 0;
            const uint32_t next = k0 + BATCH + i;
            ahead[i] = next < count ? ids[next] : 0u;
            if (k0 + i >= count) continue;
            // ',' between the tokens of a P-line and '+' / '-' behind each, '>' / '<' in front of a W-line's
            token[i] = (node[i] >> 1) < 100000000u ? make_token_short(node[i], p_lines != 0, k0 + i == first_at) : make_token(node[i], p_lines != 0, k0 + i == first_at);
            digits[i] = token[i].len;
            len += token[i].len;
        }
        uint32_t pos, total;
        BlockScan(scan_storage).ExclusiveSum(len, pos, total);
        uint8_t *const to = text + cursor;
        const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(to) & 15u);   // the batch's text lies at stage[mis ...]: LDS and memory are aligned alike
        uint8_t *w = stage + mis + pos;
#pragma unroll
        for (uint32_t i = 0; i < PER_THREAD; i++) {
            if (digits[i] == 0) continue;
            const uint32_t at = static_cast<uint32_t>(w - stage);
            uint32_t spread[4], *const dwords = reinterpret_cast<uint32_t *>(stage + (at & ~3u));
            spread_token(token[i], at & 3u, spread);
            __hip_atomic_fetch_or(dwords, spread[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_or(dwords + 1, spread[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_or(dwords + 2, spread[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (spread[3] != 0) __hip_atomic_fetch_or(dwords + 3, spread[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            w += token[i].len;
        }
        __syncthreads();
        const uint32_t end = mis + total;
        uint8_t *const aligned = to - mis;
        for (uint32_t lo = 16 * t; lo < end; lo += 16 * FORMAT_THREADS) {
            if (lo >= mis && lo + 16 <= end) {
                __builtin_nontemporal_store(*reinterpret_cast<const u32x4 *>(stage + lo), reinterpret_cast<u32x4 *>(aligned + lo));
            } else {
                const uint32_t from = lo < mis ? mis : lo, upto = lo + 16 < end ? lo + 16 : end;
                for (uint32_t q = from; q < upto; q++) aligned[q] = stage[q];
            }
            *reinterpret_cast<u32x4 *>(stage + lo) = u32x4{0u, 0u, 0u, 0u};
        }
        cursor += total;
        __syncthreads();
    }
    // trailer: "\t*\n" for P-lines (src/bin/gbunzip.rs:476), "\n" for W-lines (:548)
    if ((plan.flags & 2u) && t == 0) {
        if (p_lines) { text[cursor] = '\t'; text[cursor + 1] = '*'; text[cursor + 2] = '\n'; }
        else text[cursor] = '\n';
    }
}

// What position k of a path is: 0 = continues the segment of position k - 1, 1 = first node of a segment (a token),
// 2 = neither (the path is not a concatenation of whole segments here).
__device__ __forceinline__ uint32_t classify_position(const SegmentTables &t, const uint32_t *nodes, uint64_t begin, uint64_t k, uint32_t &segment) {
    const uint32_t node = nodes[k], id = node >> 1, rev = node & 1u;
    segment = 0;
    if (id >= t.mapping_len) return 2;
    const uint32_t s = t.seg_of[id];
    if (s == 0xFFFFFFFFu) return 2;
    segment = s;
    const uint32_t lo = t.seg_start[s], hi = t.seg_start[s + 1];
    const bool first = rev ? (id == hi - 1) : (id == lo);
    if (k == begin) return first && t.node_real[id] ? 1u : 2u;
    const uint32_t prev = nodes[k - 1], pid = prev >> 1, prev_rev = prev & 1u;
    if (pid >= t.mapping_len) return 2;
    const uint32_t ps = t.seg_of[pid];
    if (ps == 0xFFFFFFFFu) return 2;
    const bool prev_last = prev_rev ? (pid == t.seg_start[ps]) : (pid == t.seg_start[ps + 1] - 1);
    if (first && prev_last) return t.node_real[id] ? 1u : 2u;
    if (!first && !prev_last && rev == prev_rev && s == ps && id == (rev ? pid - 1 : pid + 1)) return 0;
    return 2;
}

// One wave per chunk, translation graphs: text bytes of the segment tokens, summed segment lengths, positions that fit no segment.
__global__ void __launch_bounds__(256) k_chunk_stats_segments(const uint64_t *offsets, const uint32_t *nodes, uint64_t n, const uint64_t *chunk_first, const uint32_t *chunk_path,
                                                               uint64_t chunks_cap, SegmentTables t, int p_lines, uint64_t *chunk_text, uint64_t *chunk_seq,
                                                               uint64_t *chunk_bad) {
    const uint64_t c = blockIdx.x * static_cast<uint64_t>(blockDim.x / WAVE) + threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    if (c >= chunks_cap) return;
    if (c >= chunk_first[n]) { if (lane == 0) { chunk_text[c] = 0; chunk_seq[c] = 0; chunk_bad[c] = 0; } return; }
    const ChunkRange r = chunk_range(chunk_first, chunk_path, offsets, c);
    uint64_t text = 0, labels = 0;
    uint32_t bad = 0;
    for (uint64_t k = r.lo + lane; k < r.hi; k += WAVE) {
        uint32_t s;
        const uint32_t kind = classify_position(t, nodes, r.begin, k, s);
        if (kind == 2) bad = 1;
        if (kind == 1) {
            text += (t.name_off[s + 1] - t.name_off[s]) + 1 + ((p_lines && k > r.begin) ? 1 : 0);
            labels += t.seq_len[s];
        }
    }
    for (int d = WAVE / 2; d > 0; d >>= 1) { text += __shfl_down(text, d, WAVE); labels += __shfl_down(labels, d, WAVE); bad |= __shfl_down(bad, d, WAVE); }
    if (lane == 0) { chunk_text[c] = text; chunk_seq[c] = labels; chunk_bad[c] = bad; }
}

// One workgroup per chunk, translation graphs.  Lines of flagged paths are left to the host.
__global__ void __launch_bounds__(FORMAT_THREADS) k_format_chunks_segments(const uint64_t *offsets, const uint32_t *nodes, uint64_t n, const uint64_t *chunk_first, const uint32_t *chunk_path,
                                                                            const uint64_t *text_before, SegmentTables t, int p_lines, const uint8_t *valid,
                                                                            const uint64_t *line_start, const uint64_t *seq_ids, LineHeaders hdr,
                                                                            const uint64_t *line_end, uint8_t *out) {
    using BlockScan = hipcub::BlockScan<uint32_t, FORMAT_THREADS>;
    __shared__ typename BlockScan::TempStorage scan_storage;
    if (blockIdx.x >= chunk_first[n]) return;
    const ChunkRange r = chunk_range(chunk_first, chunk_path, offsets, blockIdx.x);
    if (!valid[r.path]) return;
    const uint32_t tid = threadIdx.x;
    uint8_t *line = out + line_start[r.path];
    const uint64_t header_len = line_header(hdr, seq_ids[r.path] >> 1, line_end, r.path, r.first, line, tid, FORMAT_THREADS);
    uint64_t cursor = header_len + (text_before[blockIdx.x] - text_before[chunk_first[r.path]]);
    for (uint64_t base = r.lo; base < r.hi; base += FORMAT_THREADS) {
        const uint64_t k = base + tid;
        uint32_t len = 0, s = 0, name_len = 0;
        bool token = false, rev = false;
        if (k < r.hi) {
            token = classify_position(t, nodes, r.begin, k, s) == 1;
            if (token) {
                rev = (nodes[k] & 1u) != 0;
                name_len = static_cast<uint32_t>(t.name_off[s + 1] - t.name_off[s]);
                len = name_len + 1 + ((p_lines && k > r.begin) ? 1 : 0);
            }
        }
        uint32_t pos, total;
        BlockScan(scan_storage).ExclusiveSum(len, pos, total);
        if (token) {
            uint8_t *w = line + cursor + pos;
            if (p_lines) { if (k > r.begin) *w++ = ','; }
            else *w++ = rev ? '<' : '>';
            const uint8_t *name = t.names + t.name_off[s];
            for (uint32_t j = 0; j < name_len; j++) w[j] = name[j];
            if (p_lines) w[name_len] = rev ? '-' : '+';
        }
        cursor += total;
        __syncthreads();
    }
    if (r.last && tid == 0) {
        if (p_lines) { line[cursor] = '\t'; line[cursor + 1] = '*'; line[cursor + 2] = '\n'; }
        else line[cursor] = '\n';
    }
}

// ---- GBZ::segment_path as data (src/gbz.rs:477-489; SegmentPathIter 1098-1169) ------------------------------------------------------------
// One wave per chunk: the segment tokens of the chunk (positions that are the first node of a segment in the direction of travel) and
// whether some position fits no segment.
__global__ void __launch_bounds__(256) k_segment_chunk_tokens(const uint64_t *offsets, const uint32_t *nodes, uint64_t n, const uint64_t *chunk_first, const uint32_t *chunk_path,
                                                               uint64_t chunks_cap, SegmentTables t, uint64_t *chunk_tokens, uint64_t *chunk_bad) {
    const uint64_t c = blockIdx.x * static_cast<uint64_t>(blockDim.x / WAVE) + threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    if (c >= chunks_cap) return;
    if (c >= chunk_first[n]) { if (lane == 0) { chunk_tokens[c] = 0; chunk_bad[c] = 0; } return; }
    const ChunkRange r = chunk_range(chunk_first, chunk_path, offsets, c);
    uint64_t tokens = 0;
    uint32_t bad = 0;
    for (uint64_t k = r.lo + lane; k < r.hi; k += WAVE) {
        uint32_t s;
        const uint32_t kind = classify_position(t, nodes, r.begin, k, s);
        if (kind == 2) bad = 1;
        if (kind == 1) tokens++;
    }
    for (int d = WAVE / 2; d > 0; d >>= 1) { tokens += __shfl_down(tokens, d, WAVE); bad |= __shfl_down(bad, d, WAVE); }
    if (lane == 0) { chunk_tokens[c] = tokens; chunk_bad[c] = bad; }
}

// per row: its tokens, and whether every position fitted a whole segment (else the host replays the reference's iterator on the row)
__global__ void __launch_bounds__(256) k_segment_row_tokens(const uint64_t *chunk_first, uint64_t n, const uint64_t *tokens_before, const uint64_t *bad_before, uint64_t *row_tokens, uint8_t *valid) {
    const uint64_t p = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (p >= n) return;
    const uint64_t a = chunk_first[p], b = chunk_first[p + 1];
    row_tokens[p] = tokens_before[b] - tokens_before[a];
    valid[p] = bad_before[b] == bad_before[a] ? 1 : 0;
}

// One workgroup per chunk: token k of a valid row = (segment << 1) | orientation, at row_start[row] + tokens of the row in front of the chunk + its rank in the chunk
__global__ void __launch_bounds__(FORMAT_THREADS) k_segment_fill_tokens(const uint64_t *offsets, const uint32_t *nodes, uint64_t n, const uint64_t *chunk_first, const uint32_t *chunk_path,
                                                                         const uint64_t *tokens_before, SegmentTables t, const uint8_t *valid, const uint64_t *row_start, uint64_t *out) {
    using BlockScan = hipcub::BlockScan<uint32_t, FORMAT_THREADS>;
    __shared__ typename BlockScan::TempStorage scan_storage;
    if (blockIdx.x >= chunk_first[n]) return;
    const ChunkRange r = chunk_range(chunk_first, chunk_path, offsets, blockIdx.x);
    if (!valid[r.path]) return;
    uint64_t cursor = row_start[r.path] + (tokens_before[blockIdx.x] - tokens_before[chunk_first[r.path]]);
    for (uint64_t base = r.lo; base < r.hi; base += FORMAT_THREADS) {
        const uint64_t k = base + threadIdx.x;
        uint32_t s = 0, is_token = 0;
        if (k < r.hi) is_token = classify_position(t, nodes, r.begin, k, s) == 1 ? 1u : 0u;
        uint32_t pos, total;
        BlockScan(scan_storage).ExclusiveSum(is_token, pos, total);
        if (is_token) out[cursor + pos] = (static_cast<uint64_t>(s) << 1) | (nodes[k] & 1u);
        cursor += total;
        __syncthreads();
    }
}

}  // namespace

void launch_chunk_plan(const uint64_t *d_offsets, uint64_t n, uint64_t chunks_cap, uint64_t *d_chunk_counts, uint64_t *d_chunk_first, uint32_t *d_chunk_path, void *d_temp,
                       size_t temp_bytes, hipStream_t s, uint64_t scan_piece) {
    hipLaunchKernelGGL(k_chunk_counts, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, d_offsets, n, d_chunk_counts);
    launch_scan(d_chunk_counts, d_chunk_first, n, d_temp, temp_bytes, s, scan_piece);
    hipLaunchKernelGGL(k_chunk_paths, dim3(static_cast<unsigned>((chunks_cap + 255) / 256)), dim3(256), 0, s, d_chunk_first, n, chunks_cap, d_chunk_path);
}

void launch_chunk_stats(const ChunkedRows &r, const uint32_t *d_label_len, uint64_t n_labels, uint32_t first_node, int p_lines, uint64_t *d_chunk_text, uint64_t *d_chunk_seq,
                        hipStream_t s) {
    hipLaunchKernelGGL(k_chunk_stats, dim3(static_cast<unsigned>((r.chunks_cap + 3) / 4)), dim3(256), 0, s, r.offsets, r.nodes, r.n, r.chunk_first, r.chunk_path, r.chunks_cap,
                       d_label_len, n_labels, first_node, p_lines, d_chunk_text, d_chunk_seq);
}

void launch_chunk_stats_segments(const ChunkedRows &r, const SegmentTables &t, int p_lines, uint64_t *d_chunk_text, uint64_t *d_chunk_seq, uint64_t *d_chunk_bad, hipStream_t s) {
    hipLaunchKernelGGL(k_chunk_stats_segments, dim3(static_cast<unsigned>((r.chunks_cap + 3) / 4)), dim3(256), 0, s, r.offsets, r.nodes, r.n, r.chunk_first, r.chunk_path,
                       r.chunks_cap, t, p_lines, d_chunk_text, d_chunk_seq, d_chunk_bad);
}

void launch_line_sizes(const uint64_t *d_seq_ids, const uint64_t *d_chunk_first, uint64_t n, const uint64_t *d_text_before, const uint64_t *d_seq_before,
                       const uint64_t *d_bad_before, const LineHeaders &hdr, int p_lines, uint64_t *d_line_len, uint64_t *d_line_end, uint8_t *d_valid, hipStream_t s) {
    hipLaunchKernelGGL(k_line_sizes, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, d_seq_ids, d_chunk_first, n, d_text_before, d_seq_before, d_bad_before, hdr,
                       p_lines, d_line_len, d_line_end, d_valid);
}

void launch_line_sizes_cached(const uint64_t *d_offsets, const uint64_t *d_seq_ids, uint64_t n, const LineCache &cache, const LineHeaders &hdr, int p_lines, uint64_t *d_line_len,
                              uint64_t *d_line_end, hipStream_t s) {
    hipLaunchKernelGGL(k_line_sizes_cached, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, d_offsets, d_seq_ids, n, cache, hdr, p_lines, d_line_len, d_line_end);
}

void launch_plan_chunks(const ChunkedRows &r, const uint64_t *d_text_before, int p_lines, const uint64_t *d_line_start, const uint64_t *d_seq_ids, const LineHeaders &hdr,
                        const uint64_t *d_line_end, const LineCache &cache, ChunkPlan *d_plans, hipStream_t s) {
    hipLaunchKernelGGL(k_plan_chunks, dim3(static_cast<unsigned>((r.chunks_cap + 255) / 256)), dim3(256), 0, s, r.offsets, r.n, r.chunk_first, r.chunk_path, r.chunks_cap,
                       d_text_before, p_lines, d_line_start, d_seq_ids, hdr, d_line_end, cache, d_plans);
}

void launch_format_chunks(const ChunkedRows &r, const ChunkPlan *d_plans, int p_lines, const uint64_t *d_seq_ids, const LineHeaders &hdr, const uint64_t *d_line_end,
                          uint8_t *d_out, hipStream_t s) {
    const auto kernel = k_format_chunks<4>;   // (eight positions per thread: five waves per SIMD, 23 % slower)
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(r.chunks_cap)), dim3(FORMAT_THREADS), 0, s, r.nodes, r.n, r.chunk_first, d_plans, p_lines, d_seq_ids, hdr, d_line_end,
                       d_out);
}

void launch_format_chunks_segments(const ChunkedRows &r, const uint64_t *d_text_before, const SegmentTables &t, int p_lines, const uint8_t *d_valid,
                                   const uint64_t *d_line_start, const uint64_t *d_seq_ids, const LineHeaders &hdr, const uint64_t *d_line_end, uint8_t *d_out, hipStream_t s) {
    hipLaunchKernelGGL(k_format_chunks_segments, dim3(static_cast<unsigned>(r.chunks_cap)), dim3(FORMAT_THREADS), 0, s, r.offsets, r.nodes, r.n, r.chunk_first, r.chunk_path,
                       d_text_before, t, p_lines, d_valid, d_line_start, d_seq_ids, hdr, d_line_end, d_out);
}

void launch_segment_chunk_tokens(const ChunkedRows &r, const SegmentTables &t, uint64_t *d_chunk_tokens, uint64_t *d_chunk_bad, hipStream_t s) {
    hipLaunchKernelGGL(k_segment_chunk_tokens, dim3(static_cast<unsigned>((r.chunks_cap + 3) / 4)), dim3(256), 0, s, r.offsets, r.nodes, r.n, r.chunk_first, r.chunk_path,
                       r.chunks_cap, t, d_chunk_tokens, d_chunk_bad);
}

void launch_segment_row_tokens(const uint64_t *d_chunk_first, uint64_t n, const uint64_t *d_tokens_before, const uint64_t *d_bad_before, uint64_t *d_row_tokens,
                               uint8_t *d_valid, hipStream_t s) {
    hipLaunchKernelGGL(k_segment_row_tokens, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, d_chunk_first, n, d_tokens_before, d_bad_before, d_row_tokens, d_valid);
}

void launch_segment_fill_tokens(const ChunkedRows &r, const uint64_t *d_tokens_before, const SegmentTables &t, const uint8_t *d_valid, const uint64_t *d_row_start,
                                uint64_t *d_out, hipStream_t s) {
    hipLaunchKernelGGL(k_segment_fill_tokens, dim3(static_cast<unsigned>(r.chunks_cap)), dim3(FORMAT_THREADS), 0, s, r.offsets, r.nodes, r.n, r.chunk_first, r.chunk_path,
                       d_tokens_before, t, d_valid, d_row_start, d_out);
}

}  // namespace gbwt_hip
