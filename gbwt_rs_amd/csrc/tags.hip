// tags.hip -- gbz-extract's `tag-array` mode (src/bin/gbz-extract.rs:296-482): the graph position of every entry of a suffix array that an
// external tool built over the text `sequences` mode wrote.
//
// The text of paths p_0 .. p_{n-1} is the forward bases of p_0, one endmarker, the bases of p_1, one endmarker, ...  The tag of text position t
// (extract_path / encode_start, :346-371) is 0 for an endmarker and otherwise ((v << 11) | (o << 10)) + w for the base w bases (in reading
// direction, also on a reverse node) behind the first base of the visit of node v in orientation o that t falls into.  With the GBWT-encoded
// node 2 v + o of the walk that is (node << 10) + w.  It is a plain 64-bit ADDITION, as in the reference, which does not guard labels longer
// than 1 024 bases (its FIXME): there w carries into the orientation bit and the node id, and so it does here.  Nodes are nodes, never
// segments.  TAG[i] = tag(SA[i]): the reference gets there with two sorts of (index, value) pairs, which compute exactly this gather when
// the values read are a permutation of 0 .. expected_len - 1; for other input the reference's result is unspecified and ours is the gather.
// A value >= expected_len is reported (GBWT_HIP_INVALID_DATA) and never read through.
//
// PLAN (kept on the workspace while the list of path ids stays the same): the rows are the extraction of sequences 2 p (k_walk_direct); one
// pass gives every POSITION of the text's walk -- the nodes of a row and one pseudo-position of node 0 and length 1 behind it for its endmarker
// -- its node and its label length, a scan turns the lengths into text offsets, and a sampled top level holds for every 32nd text
// offset (1 << TAG_SHIFT) the position it falls into.  12 bytes per position + 4 (8 from 2^32 positions) per 32 text offsets.
//
// GATHER (k_tags): one suffix-array value in, one tag out.  The two hints around a value bound a search over at most 33 text
// offsets (every position with bases has at least one, so a window of 32 text offsets starts at most 32 of them) -- three cache lines for
// labels of one base, one for labels of tens of bases -- then the position's offset (a line the search has just touched) and its node.
// Every thread runs four lookups in lock step, so that four dependent chains are in flight per lane; the values are loaded coalesced, the
// tags leave with non-temporal stores.  A workgroup owns a contiguous range of tiles: the tag in front of a tile is the last tag of the tile
// before it, kept in LDS, so that the runs (TAG[i] != TAG[i - 1]) are counted in the same pass, with one extra lookup and one atomic per workgroup.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "batch_writer.hpp"
#include "capi_internal.hpp"

using namespace gbwt_hip;

namespace {

constexpr uint32_t TAG_SHIFT = 5;                                   // one hint per 32 text offsets
constexpr uint32_t TAG_THREADS = 256, TAG_PER = 4, TAG_TILE = TAG_THREADS * TAG_PER;
constexpr uint64_t SCAN_PIECE = uint64_t(1) << 30;                  // (launch_scan counts in int)

// What a request leaves behind: the runs counted so far, the last tag of the batches (two slots in turn: a batch reads the one its
// predecessor wrote while its own last workgroup writes the other), and whether a value was out of range.
struct TagState { unsigned long long runs; uint64_t last[2]; uint32_t bad, reserved; };
static_assert(sizeof(TagState) == 32, "copied as a whole");

// The position map of a plan as the kernels see it
template <class H> struct TagMap { const H *top; const uint64_t *off; const uint32_t *node; uint64_t text_len; };

// Node and label length of every position: position q of row k (the k with offsets[k] + k <= q <= offsets[k + 1] + k) is the walk's node
// offsets[k] + (q - offsets[k] - k), the last one of the row its endmarker.
__global__ void __launch_bounds__(256) k_tag_positions(const uint64_t *offsets, const uint32_t *nodes, uint64_t n, uint64_t positions, Labels L, uint32_t *pos_node,
                                                        uint64_t *pos_len) {
    const uint64_t q = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (q >= positions) return;
    uint64_t lo = 0, hi = n - 1;                     // the last row that starts at or before q
    while (lo < hi) { const uint64_t mid = lo + (hi - lo + 1) / 2; if (offsets[mid] + mid <= q) lo = mid; else hi = mid - 1; }
    const uint64_t j = q - lo;                       // index into the walk's nodes, or the end of the row
    if (j == offsets[lo + 1]) { pos_node[q] = 0; pos_len[q] = 1; return; }
    const uint32_t node = nodes[j];
    uint64_t a, b;
    label_of(L, node, a, b);
    pos_node[q] = node;
    pos_len[q] = b - a;
}

// launch_scan in pieces (it counts in int, and clears the word in front of what it writes): a piece starts from the sum in front of it, which is
// added to its first length and put back where the scan of the piece has cleared it
__global__ void k_tag_carry(uint64_t *pos_len, uint64_t *pos_off, uint64_t at, uint64_t *saved, int restore) {
    if (restore) { pos_off[at] = *saved; return; }
    *saved = pos_off[at];
    pos_len[at] += *saved;
}

// Text offset of every row, and the text length behind the last
__global__ void __launch_bounds__(256) k_tag_rows(const uint64_t *offsets, uint64_t n, const uint64_t *pos_off, uint64_t positions, uint64_t *rows) {
    const uint64_t k = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (k > n) return;
    rows[k] = k < n ? pos_off[offsets[k] + k] : pos_off[positions];
}

// top[h] = the last position that starts at or before text offset h << TAG_SHIFT (the one that holds it: a position without bases never is the
// last one); top[hints - 1] = the last position, the bound of the searches in the last window.
template <class H>
__global__ void __launch_bounds__(256) k_tag_top(const uint64_t *pos_off, uint64_t positions, uint64_t hints, H *top) {
    const uint64_t h = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (h >= hints) return;
    if (h + 1 == hints) { top[h] = static_cast<H>(positions - 1); return; }
    const uint64_t t = h << TAG_SHIFT;
    uint64_t lo = 0, hi = positions - 1;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo + 1) / 2; if (pos_off[mid] <= t) lo = mid; else hi = mid - 1; }
    top[h] = static_cast<H>(lo);
}

// The tag of one text offset t < text_len (the lookup of the gather kernel, alone: the tag in front of a workgroup's first tile)
template <class H>
__device__ __forceinline__ uint64_t tag_of(const TagMap<H> &m, uint64_t t) {
    uint64_t lo = m.top[t >> TAG_SHIFT], hi = m.top[(t >> TAG_SHIFT) + 1];
    while (lo < hi) { const uint64_t mid = lo + (hi - lo + 1) / 2; if (m.off[mid] <= t) lo = mid; else hi = mid - 1; }
    return (static_cast<uint64_t>(m.node[lo]) << 10) + (t - m.off[lo]);
}

// See the top of the file.  Entry base + 256 i + t of a tile is lookup i of thread t.  has_prev: a batch in front of this one has left its last
// tag in state->last[parity ^ 1]; without, entry 0 counts as the start of a run.
template <class H>
__global__ void __launch_bounds__(TAG_THREADS) k_tags(const uint64_t *__restrict__ sa, uint64_t count, TagMap<H> m, uint64_t *__restrict__ tags, TagState *state,
                                                       uint32_t has_prev, uint32_t parity) {
    __shared__ uint64_t tile[TAG_TILE + 1];          // tile[0]: the tag in front of the tile
    const uint32_t t = threadIdx.x;
    const uint64_t tiles = (count + TAG_TILE - 1) / TAG_TILE, share = (tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t first = blockIdx.x * share, end = first + share < tiles ? first + share : tiles;
    if (first >= end) return;
    uint32_t runs = 0, bad = 0;
    const bool opens = first == 0 && !has_prev;      // entry 0 has nothing in front of it
    if (t == 0) {
        uint64_t front = 0;
        if (first != 0) {
            const uint64_t v = sa[first * TAG_TILE - 1];
            if (v < m.text_len) front = tag_of(m, v);
        } else if (has_prev) front = state->last[parity ^ 1u];
        tile[0] = front;
    }
    for (uint64_t tl = first; tl < end; tl++) {
        const uint64_t base = tl * TAG_TILE;
        uint64_t v[TAG_PER], lo[TAG_PER], hi[TAG_PER];
        bool live[TAG_PER], ok[TAG_PER];
#pragma unroll
        for (uint32_t i = 0; i < TAG_PER; i++) {
            const uint64_t at = base + i * TAG_THREADS + t;
            live[i] = at < count;
            v[i] = live[i] ? __builtin_nontemporal_load(sa + at) : 0;
            ok[i] = v[i] < m.text_len;               // (text_len != 0: the host launches nothing for an empty text)
            if (!ok[i]) { bad = 1; v[i] = 0; }       // never read through: the lookup of such a lane is that of offset 0
        }
#pragma unroll
        for (uint32_t i = 0; i < TAG_PER; i++) { const uint64_t h = v[i] >> TAG_SHIFT; lo[i] = m.top[h]; hi[i] = m.top[h + 1]; }
        for (;;) {                                   // the four searches in lock step: every round loads for all of them
            bool more = false;
            uint64_t mid[TAG_PER], o[TAG_PER];
#pragma unroll
            for (uint32_t i = 0; i < TAG_PER; i++) { mid[i] = lo[i] + (hi[i] - lo[i] + 1) / 2; o[i] = m.off[mid[i]]; }
#pragma unroll
            for (uint32_t i = 0; i < TAG_PER; i++) {
                if (lo[i] < hi[i]) { if (o[i] <= v[i]) lo[i] = mid[i]; else hi[i] = mid[i] - 1; }
                more |= lo[i] < hi[i];
            }
            if (!more) break;
        }
        uint64_t o[TAG_PER], tag[TAG_PER];
        uint32_t node[TAG_PER];
#pragma unroll
        for (uint32_t i = 0; i < TAG_PER; i++) { o[i] = m.off[lo[i]]; node[i] = m.node[lo[i]]; }
#pragma unroll
        for (uint32_t i = 0; i < TAG_PER; i++) {
            tag[i] = ok[i] ? (static_cast<uint64_t>(node[i]) << 10) + (v[i] - o[i]) : 0;
            tile[1 + i * TAG_THREADS + t] = tag[i];
            if (live[i] && ok[i]) __builtin_nontemporal_store(tag[i], tags + base + i * TAG_THREADS + t);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < TAG_PER; i++) {
            const uint32_t at = i * TAG_THREADS + t;
            if (live[i]) runs += (opens && base + at == 0) || tag[i] != tile[at] ? 1u : 0u;
        }
        const uint64_t carry = tile[TAG_TILE];
        if (tl + 1 == tiles) {                       // the last entry of the batch leaves its tag for the next one
            const uint64_t last = count - 1 - base;
            if (t == last % TAG_THREADS) state->last[parity] = tile[1 + last];
        }
        __syncthreads();
        if (t == 0) tile[0] = carry;
    }
    for (int d = 32; d > 0; d >>= 1) { runs += __shfl_down(runs, d, 64); bad |= __shfl_down(bad, d, 64); }
    __shared__ uint32_t wave_runs[TAG_THREADS / 64], wave_bad[TAG_THREADS / 64];
    if (t % 64 == 0) { wave_runs[t / 64] = runs; wave_bad[t / 64] = bad; }
    __syncthreads();
    if (t == 0) {
        uint32_t r = 0, b = 0;
        for (uint32_t w = 0; w < TAG_THREADS / 64; w++) { r += wave_runs[w]; b |= wave_bad[w]; }
        if (r) atomicAdd(&state->runs, static_cast<unsigned long long>(r));
        if (b) atomicOr(&state->bad, 1u);
    }
}

struct OutOfMemory { std::string what; };

// Growing `buffers` to `need` bytes each: what that takes beyond what they hold must be free on the device (a buffer that grows gives its
// old memory back first)
void require_fits(std::initializer_list<std::pair<const DeviceBuffer *, uint64_t>> buffers, const char *what) {
    uint64_t more = 0, back = 0, total = 0;
    for (const auto &b : buffers) { total += b.second; if (b.second > b.first->bytes) { more += b.second; back += b.first->bytes; } }
    size_t free_bytes = 0, all = 0;
    HIP_CHECK(hipMemGetInfo(&free_bytes, &all));
    if (more > static_cast<uint64_t>(free_bytes) + back)
        throw OutOfMemory{std::string(what) + " needs " + std::to_string(total) + " bytes of device memory, " + std::to_string(more - back) + " more than the workspace holds for it; " +
                          std::to_string(free_bytes) + " are free"};
}

void drop_plan(gbwt_hip_workspace *ws) { ws->tags.plan_key.drop(); ws->tags.timed = false; ws->tags.rows.clear(); ws->tags.positions = 0; ws->tags.text_len = 0; }

// The plan of a list of path ids (see the top of the file), made unless the workspace holds it
gbwt_hip_status tags_plan(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n) {
    if (!ix || !ws || ws->index != ix) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    if (n && !path_ids) return fail(GBWT_HIP_BAD_ARGUMENT, "null path_ids");
    if (ws->tags.plan_key.matches({{path_ids, n * sizeof(uint64_t)}}, {})) {
        ws->tags.gather_ms = 0;
        return GBWT_HIP_OK;
    }
    drop_plan(ws);
    try {
        require_bases_capable(ix);
        const HostIndex &h = ix->host;
        std::vector<uint64_t> seq_ids(n);
        for (uint64_t k = 0; k < n; k++) {
            if (path_ids[k] >= (~uint64_t(0)) / 2 || 2 * path_ids[k] >= h.sequences) return fail(GBWT_HIP_BAD_ARGUMENT, "path id out of range: " + std::to_string(path_ids[k]));
            seq_ids[k] = 2 * path_ids[k];            // GBZ::path(id, Forward) = sequence 2 id (support::encode_path)
        }
        HIP_CHECK(hipSetDevice(ix->device));
        hipStream_t s = ws->stream;
        ws->tags.ev.ensure();
        ws->tags.state.reserve(sizeof(TagState));
        ws->tags.walk_ms = ws->tags.plan_ms = ws->tags.gather_ms = 0;
        if (n == 0) {                                // an empty text: nothing to look anything up in
            ws->tags.rows.assign(1, 0);
            ws->tags.plan_key.store({{nullptr, 0}}, {});
            ws->tags.timed = true;
            return GBWT_HIP_OK;
        }
        ensure_labels(ix);
        gbwt_hip_paths paths{};
        const gbwt_hip_status st = gbwt_hip_extract_device(ix, ws, seq_ids.data(), n, &paths);
        if (st != GBWT_HIP_OK) return st;
        HIP_CHECK(hipEventElapsedTime(&ws->tags.walk_ms, ws->extract.ev[0], ws->extract.ev[1]));
        const uint64_t positions = paths.total + n;
        // GBWT_HIP_TAG_SCAN_PIECE (positions per launch of the scan) and GBWT_HIP_TAG_WIDE (64-bit hints whatever the size) let tests reach what
        // only plans of 2^30 and 2^32 positions reach otherwise; read when a plan is made
        uint64_t scan_piece = SCAN_PIECE;
        if (const char *v = std::getenv("GBWT_HIP_TAG_SCAN_PIECE")) scan_piece = std::min<uint64_t>(SCAN_PIECE, std::max<uint64_t>(1024, std::strtoull(v, nullptr, 10)));
        const char *force_wide = std::getenv("GBWT_HIP_TAG_WIDE");
        const bool wide = positions > 0xFFFFFFFFull || (force_wide && std::atoi(force_wide) != 0);
        DeviceBuffer lengths;                        // the label lengths in front of the scan: scratch of the plan
        require_fits({{&ws->tags.node, positions * sizeof(uint32_t)}, {&ws->tags.off, (positions + 1) * sizeof(uint64_t)}, {&lengths, positions * sizeof(uint64_t)}}, "the tag plan");
        ws->tags.node.reserve(positions * sizeof(uint32_t));
        ws->tags.off.reserve((positions + 1) * sizeof(uint64_t));
        lengths.reserve(positions * sizeof(uint64_t));
        const size_t tb = scan_temp_bytes(std::min(positions, scan_piece));
        ws->scratch.scan_temp.reserve(std::max<size_t>(tb, 16));
        ws->scratch.a.reserve((n + 1) * sizeof(uint64_t));
        uint64_t *d_len = lengths.as<uint64_t>(), *d_off = ws->tags.off.as<uint64_t>(), *d_rows = ws->scratch.a.as<uint64_t>();
        const auto blocks = [](uint64_t items) { return dim3(static_cast<unsigned>((items + 255) / 256)); };
        HIP_CHECK(hipEventRecord(ws->tags.ev[0], s));
        hipLaunchKernelGGL(k_tag_positions, blocks(positions), dim3(256), 0, s, paths.d_offsets, paths.d_nodes, n, positions, labels_of(ix), ws->tags.node.as<uint32_t>(), d_len);
        for (uint64_t at = 0; at < positions; at += scan_piece) {
            const uint64_t piece = std::min(scan_piece, positions - at);
            uint64_t *saved = ws->tags.state.as<TagState>()->last;          // (a word nobody reads before the next request clears the state)
            if (at != 0) hipLaunchKernelGGL(k_tag_carry, dim3(1), dim3(1), 0, s, d_len, d_off, at, saved, 0);
            launch_scan(d_len + at, d_off + at, piece, ws->scratch.scan_temp.ptr, tb, s);
            if (at != 0) hipLaunchKernelGGL(k_tag_carry, dim3(1), dim3(1), 0, s, d_len, d_off, at, saved, 1);
        }
        hipLaunchKernelGGL(k_tag_rows, blocks(n + 1), dim3(256), 0, s, paths.d_offsets, n, d_off, positions, d_rows);
        ws->tags.rows.resize(n + 1);
        HIP_CHECK(hipMemcpyAsync(ws->tags.rows.data(), d_rows, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));          // the one wait of a plan: the text length sizes the top level
        HIP_CHECK(hipGetLastError());
        lengths.release();
        const uint64_t text_len = ws->tags.rows[n], hints = ((text_len - 1) >> TAG_SHIFT) + 2;
        const uint64_t top_bytes = hints * (wide ? sizeof(uint64_t) : sizeof(uint32_t));
        require_fits({{&ws->tags.top, top_bytes}}, "the top level of the tag plan");
        ws->tags.top.reserve(top_bytes);
        if (wide) hipLaunchKernelGGL(k_tag_top<uint64_t>, blocks(hints), dim3(256), 0, s, d_off, positions, hints, ws->tags.top.as<uint64_t>());
        else hipLaunchKernelGGL(k_tag_top<uint32_t>, blocks(hints), dim3(256), 0, s, d_off, positions, hints, ws->tags.top.as<uint32_t>());
        HIP_CHECK(hipEventRecord(ws->tags.ev[1], s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventElapsedTime(&ws->tags.plan_ms, ws->tags.ev[0], ws->tags.ev[1]));
        ws->tags.positions = positions;
        ws->tags.text_len = text_len;
        ws->tags.wide = wide;
        ws->tags.plan_key.store({{path_ids, n * sizeof(uint64_t)}}, {});
        ws->tags.timed = true;
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const OutOfMemory &e) {
        return fail(GBWT_HIP_CAPACITY, e.what);
    } catch (const HipError &e) {
        return status_of(e, "the tag plan");
    }
}

// One batch of the gather on the workspace's stream (nothing is waited for): tags[i] = tag(sa[i]) for i < count, runs and flag into tag_state
void launch_tags(gbwt_hip_workspace *ws, const uint64_t *d_sa, uint64_t count, uint64_t *d_tags, bool has_prev, uint32_t parity) {
    int cus = 0;
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ws->index->device));
    const uint64_t tiles = (count + TAG_TILE - 1) / TAG_TILE;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(tiles, 8ull * static_cast<unsigned>(std::max(cus, 1))));   // eight workgroups per CU: what its registers hold
    TagState *state = ws->tags.state.as<TagState>();
    if (ws->tags.wide) {
        const TagMap<uint64_t> m{ws->tags.top.as<uint64_t>(), ws->tags.off.as<uint64_t>(), ws->tags.node.as<uint32_t>(), ws->tags.text_len};
        hipLaunchKernelGGL(k_tags<uint64_t>, dim3(grid), dim3(TAG_THREADS), 0, ws->stream, d_sa, count, m, d_tags, state, has_prev ? 1u : 0u, parity);
    } else {
        const TagMap<uint32_t> m{ws->tags.top.as<uint32_t>(), ws->tags.off.as<uint64_t>(), ws->tags.node.as<uint32_t>(), ws->tags.text_len};
        hipLaunchKernelGGL(k_tags<uint32_t>, dim3(grid), dim3(TAG_THREADS), 0, ws->stream, d_sa, count, m, d_tags, state, has_prev ? 1u : 0u, parity);
    }
    HIP_CHECK(hipGetLastError());
}

// A whole request for `count` values in HBM: state cleared, one launch, the host waits; INVALID_DATA for a value out of range
gbwt_hip_status gather_once(gbwt_hip_workspace *ws, const uint64_t *d_sa, uint64_t count, uint64_t *d_tags, uint64_t *runs) {
    if (runs) *runs = 0;
    if (count == 0) return GBWT_HIP_OK;
    if (ws->tags.text_len == 0) return fail(GBWT_HIP_INVALID_DATA, "suffix array value out of range: the text of no paths is empty");
    hipStream_t s = ws->stream;
    TagState state{};
    HIP_CHECK(hipMemsetAsync(ws->tags.state.ptr, 0, sizeof(TagState), s));
    HIP_CHECK(hipEventRecord(ws->tags.ev[0], s));
    launch_tags(ws, d_sa, count, d_tags, false, 0);
    HIP_CHECK(hipEventRecord(ws->tags.ev[1], s));
    HIP_CHECK(hipMemcpyAsync(&state, ws->tags.state.ptr, sizeof(TagState), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipEventElapsedTime(&ws->tags.gather_ms, ws->tags.ev[0], ws->tags.ev[1]));
    if (state.bad) return fail(GBWT_HIP_INVALID_DATA, "suffix array value out of range: the text has " + std::to_string(ws->tags.text_len) + " positions");
    if (runs) *runs = state.runs;
    return GBWT_HIP_OK;
}

// first tab field = path id, last tab field = bases (read_names, src/bin/gbz-extract.rs:296-318)
bool parse_number(const std::string &field, uint64_t &out) {
    if (field.empty() || field.size() > 19) return false;
    out = 0;
    for (char c : field) { if (c < '0' || c > '9') return false; out = 10 * out + static_cast<uint64_t>(c - '0'); }
    return true;
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_tags_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, const uint64_t *d_sa, uint64_t count,
                                     uint64_t *d_tags, uint64_t *runs) {
    GBWT_HIP_GUARD_BEGIN
    if (runs) *runs = 0;
    const gbwt_hip_status st = tags_plan(ix, ws, path_ids, n);
    if (st != GBWT_HIP_OK) return st;
    if (count && (!d_sa || !d_tags)) return fail(GBWT_HIP_BAD_ARGUMENT, "null suffix array / tags");
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        return gather_once(ws, d_sa, count, d_tags, runs);
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_tags(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, const uint64_t *sa, uint64_t count, uint64_t *tags,
                              uint64_t *expected_len, uint64_t *runs) {
    GBWT_HIP_GUARD_BEGIN
    if (expected_len) *expected_len = 0;
    if (runs) *runs = 0;
    const gbwt_hip_status st = tags_plan(ix, ws, path_ids, n);
    if (st != GBWT_HIP_OK) return st;
    if (expected_len) *expected_len = ws->tags.text_len;
    if (!sa && !tags) return GBWT_HIP_OK;            // the size query
    if (count && (!sa || !tags)) return fail(GBWT_HIP_BAD_ARGUMENT, "null suffix array / tags");
    if (count == 0) return GBWT_HIP_OK;
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        if (count > (~uint64_t(0)) / 16) return fail(GBWT_HIP_CAPACITY, "suffix array too large for device memory");
        require_fits({{&ws->tags.sa, count * sizeof(uint64_t)}, {&ws->tags.out, count * sizeof(uint64_t)}}, "the suffix array and its tags");
        ws->tags.sa.reserve(count * sizeof(uint64_t));
        ws->tags.out.reserve(count * sizeof(uint64_t));
        HIP_CHECK(hipMemcpyAsync(ws->tags.sa.ptr, sa, count * sizeof(uint64_t), hipMemcpyHostToDevice, ws->stream));
        const gbwt_hip_status gst = gather_once(ws, ws->tags.sa.as<uint64_t>(), count, ws->tags.out.as<uint64_t>(), runs);
        if (gst != GBWT_HIP_OK) return gst;          // (the caller's tags are untouched)
        copy_to_host(ws, tags, ws->tags.out.ptr, count * sizeof(uint64_t));
        return GBWT_HIP_OK;
    } catch (const OutOfMemory &e) {
        return fail(GBWT_HIP_CAPACITY, e.what);
    } catch (const HipError &e) {
        return status_of(e, "the suffix array");
    }
    GBWT_HIP_GUARD_END
}

// gbz-extract -m tag-array -o base (extract_tag_array, src/bin/gbz-extract.rs:408-482)
gbwt_hip_status gbwt_hip_write_tag_array(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const char *base_path, uint64_t sa_skip, uint64_t *runs) {
    GBWT_HIP_GUARD_BEGIN
    if (runs) *runs = 0;
    if (!ix || !ws || ws->index != ix || !base_path) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace / path");
    const std::string base(base_path), names_path = base + ".names", sa_path = base + ".sa", tags_path = base + ".tags";
    try {
        require_bases_capable(ix);
        // 1. the names: path id, bases
        std::vector<uint64_t> ids, lens;
        {
            FILE *f = std::fopen(names_path.c_str(), "rb");
            if (!f) return fail(GBWT_HIP_IO_ERROR, "cannot open " + names_path);
            std::string text;
            char buffer[1 << 16];
            size_t got;
            while ((got = std::fread(buffer, 1, sizeof(buffer), f)) != 0) text.append(buffer, got);
            const bool broken = std::ferror(f) != 0;
            std::fclose(f);
            if (broken) return fail(GBWT_HIP_IO_ERROR, "cannot read " + names_path);
            for (size_t at = 0; at < text.size();) {
                size_t nl = text.find('\n', at);
                if (nl == std::string::npos) nl = text.size();
                std::string line = text.substr(at, nl - at);
                if (!line.empty() && line.back() == '\r') line.pop_back();          // (BufRead::lines strips "\r\n" as well)
                at = nl + 1;
                const size_t head = line.find('\t'), tail = line.rfind('\t');
                if (head == std::string::npos) return fail(GBWT_HIP_INVALID_DATA, "Name line missing last field");   // (one field: next_back finds nothing)
                uint64_t id = 0, len = 0;
                if (!parse_number(line.substr(0, head), id) || !parse_number(line.substr(tail + 1), len))
                    return fail(GBWT_HIP_INVALID_DATA, "invalid digit found in string: " + line);
                ids.push_back(id); lens.push_back(len);
            }
        }
        if (ids.empty()) return fail(GBWT_HIP_INVALID_DATA, "No path names found");
        for (size_t k = 0; k < ids.size(); k++)      // GBZ::path gives nothing for such an id: extract_path is the endmarker alone
            if (ids[k] >= (~uint64_t(0)) / 2 || 2 * ids[k] >= ix->host.sequences)
                return fail(GBWT_HIP_INVALID_DATA, "Invalid length for path " + std::to_string(ids[k]) + ": expected " + std::to_string(lens[k]) + ", got 0 (no such path)");
        // 2. the plan, and the walked bases of every path against its line
        const gbwt_hip_status st = tags_plan(ix, ws, ids.data(), ids.size());
        if (st != GBWT_HIP_OK) return st;
        for (size_t k = 0; k < ids.size(); k++) {
            const uint64_t walked = ws->tags.rows[k + 1] - ws->tags.rows[k] - 1;
            if (walked != lens[k])
                return fail(GBWT_HIP_INVALID_DATA, "Invalid length for path " + std::to_string(ids[k]) + ": expected " + std::to_string(lens[k]) + ", got " + std::to_string(walked));
        }
        const uint64_t expected_len = ws->tags.text_len;
        // 3. the suffix array: sa_skip values skipped, expected_len read
        PositionalFile sa_file, out;
        sa_file.fd = ::open(sa_path.c_str(), O_RDONLY);
        if (sa_file.fd < 0) return fail(GBWT_HIP_IO_ERROR, "cannot open " + sa_path);
        struct stat info {};
        if (::fstat(sa_file.fd, &info) != 0) return fail(GBWT_HIP_IO_ERROR, "cannot stat " + sa_path);
        if (sa_skip > (~uint64_t(0)) / 16 || static_cast<uint64_t>(info.st_size) / sizeof(uint64_t) < sa_skip + expected_len)
            return fail(GBWT_HIP_IO_ERROR, sa_path + " is too short: " + std::to_string(sa_skip + expected_len) + " values expected, " + std::to_string(info.st_size) + " bytes found");
        uint64_t budget = uint64_t(256) << 20;
        if (const char *v = std::getenv("GBWT_HIP_TAG_BATCH_MIB")) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10)) << 20;
        const uint64_t batch = std::min<uint64_t>(std::max<uint64_t>(budget / sizeof(uint64_t), 1), expected_len);
        HIP_CHECK(hipSetDevice(ix->device));
        require_fits({{&ws->tags.sa, batch * sizeof(uint64_t)}, {&ws->tags.sa2, batch * sizeof(uint64_t)}, {&ws->tags.out, batch * sizeof(uint64_t)}, {&ws->tags.out2, batch * sizeof(uint64_t)}},
                     "the batches of the tag array");
        for (DeviceBuffer *b : {&ws->tags.sa, &ws->tags.sa2, &ws->tags.out, &ws->tags.out2}) b->reserve(batch * sizeof(uint64_t));
        std::vector<uint64_t> values(batch);
        HIP_CHECK(hipMemsetAsync(ws->tags.state.ptr, 0, sizeof(TagState), ws->stream));
        out.fd = ::open(tags_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (out.fd < 0) return fail(GBWT_HIP_IO_ERROR, "cannot create " + tags_path);
        gbwt_hip_status result = GBWT_HIP_OK;
        std::string message;
        TagState state{};
        float gather_ms = 0;
        {
            BatchWriter writer;
            writer.file = &out; writer.device = ix->device; writer.what = "tags";
            writer.start();
            hipStream_t s = ws->stream;
            int slot = 0;
            uint32_t batches = 0;
            try {
                for (uint64_t done = 0; done < expected_len; done += batch, batches++, slot ^= 1) {
                    const uint64_t cnt = std::min(batch, expected_len - done);
                    uint64_t got = 0;
                    while (got < cnt * sizeof(uint64_t)) {
                        const ssize_t r = ::pread(sa_file.fd, reinterpret_cast<char *>(values.data()) + got, cnt * sizeof(uint64_t) - got,
                                                  static_cast<off_t>((sa_skip + done) * sizeof(uint64_t) + got));
                        if (r <= 0) break;
                        got += static_cast<uint64_t>(r);
                    }
                    if (got < cnt * sizeof(uint64_t)) { result = GBWT_HIP_IO_ERROR; message = "short read from " + sa_path; break; }
                    if (!writer.acquire(slot)) { result = GBWT_HIP_IO_ERROR; break; }   // (the writer's own message, below)
                    uint64_t *d_sa = (slot == 0 ? ws->tags.sa : ws->tags.sa2).as<uint64_t>(), *d_tags = (slot == 0 ? ws->tags.out : ws->tags.out2).as<uint64_t>();
                    HIP_CHECK(hipMemcpyAsync(d_sa, values.data(), cnt * sizeof(uint64_t), hipMemcpyHostToDevice, s));
                    HIP_CHECK(hipEventRecord(ws->tags.ev[0], s));
                    launch_tags(ws, d_sa, cnt, d_tags, batches != 0, batches & 1u);
                    HIP_CHECK(hipEventRecord(ws->tags.ev[1], s));
                    HIP_CHECK(hipMemcpyAsync(&state, ws->tags.state.ptr, sizeof(TagState), hipMemcpyDeviceToHost, s));
                    HIP_CHECK(hipStreamSynchronize(s));
                    float ms = 0;
                    HIP_CHECK(hipEventElapsedTime(&ms, ws->tags.ev[0], ws->tags.ev[1]));
                    gather_ms += ms;
                    if (state.bad) {
                        result = GBWT_HIP_INVALID_DATA;
                        message = "suffix array value out of range: the text has " + std::to_string(expected_len) + " positions";
                        break;
                    }
                    writer.submit(reinterpret_cast<const char *>(d_tags), cnt * sizeof(uint64_t), slot);
                }
            } catch (const HipError &e) {
                result = GBWT_HIP_DEVICE_ERROR;
                message = std::string(e.what) + ": " + hipGetErrorString(e.err);
            }
            const gbwt_hip_status wst = writer.finish();
            if (wst != GBWT_HIP_OK && (result == GBWT_HIP_OK || message.empty())) { result = wst; message = writer.message; }
        }
        if (result == GBWT_HIP_OK && out.failed) { result = GBWT_HIP_IO_ERROR; message = "short write to " + tags_path; }
        ws->tags.gather_ms = gather_ms;
        if (result != GBWT_HIP_OK) {
            (void)::unlink(tags_path.c_str());      // nothing half written stays behind
            return fail(result, message);
        }
        if (runs) *runs = state.runs;
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const OutOfMemory &e) {
        return fail(GBWT_HIP_CAPACITY, e.what);
    } catch (const HipError &e) {
        return status_of(e, "the batches of the tag array");
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_tags_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *plan_ms, float *gather_ms) {
    GBWT_HIP_GUARD_BEGIN
    if (!ws || !ws->tags.timed) return fail(GBWT_HIP_BAD_ARGUMENT, "no timed request for tags on this workspace");
    if (walk_ms) *walk_ms = ws->tags.walk_ms;
    if (plan_ms) *plan_ms = ws->tags.plan_ms;
    if (gather_ms) *gather_ms = ws->tags.gather_ms;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

}  // extern "C"
