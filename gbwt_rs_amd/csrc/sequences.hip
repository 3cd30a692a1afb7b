// sequences.hip -- the bases of GBZ paths (gbz-extract's `sequences` mode, src/bin/gbz-extract.rs:173-194, 266-294) on top of the device extraction.
//
// The sequence of a path is the concatenation of GBZ::sequence(node) along GBZ::path(path, orientation) (src/gbz.rs:292-305), with the
// labels of reverse-oriented nodes reverse-complemented (support::reverse_complement, src/support.rs:87-110: A/C/G/T in either case to the
// upper-case complement, every other byte to N), and -- when asked for -- one endmarker byte behind every path.  A request walks the rows
// (k_walk_direct), sizes them (the line cache of the index, or a pass over the label lengths in the chunks of the line formatter), places
// the rows with a scan, and one workgroup per chunk of GFA_LINE_CHUNK positions copies the labels: a block scan over the label lengths of
// 1 024 positions at a time places the nodes in LDS, then every lane owns aligned 16-byte units of the output, finds the node of its first
// byte by a search of that prefix array and gathers the bytes.  The work is per OUTPUT byte, not per node: labels of 1 and of 1 024 bases
// keep the same lanes busy.  A unit that lies inside one node -- the common case with labels of tens of bases -- is five aligned dword
// loads and a byte shift (v_alignbyte); units across node boundaries go byte by byte.
//
// The node labels reach HBM on the first request for bases (ensure_labels), never at open.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "batch_writer.hpp"
#include "capi_internal.hpp"
#include "gfa_host.hpp"
#include "lines.hpp"

using namespace gbwt_hip;

namespace {

constexpr int WAVE = 64;
constexpr uint32_t SEQ_CHUNK = GFA_LINE_CHUNK;     // path positions per chunk (the chunks of the line formatter: launch_chunk_plan)
constexpr uint32_t BASES_THREADS = 256, PER_THREAD = 4, BATCH = BASES_THREADS * PER_THREAD;
constexpr uint64_t LABEL_PAD = 64;                 // zero bytes behind the last label (the dword loads of a unit read up to 3 bytes past it)
constexpr uint64_t REVERSE_BIT = uint64_t(1) << 63;

// support::COMPLEMENT (src/support.rs:87-99)
__host__ __device__ __forceinline__ uint8_t complement(uint32_t c) {
    switch (c) {
        case 'A': case 'a': return 'T';
        case 'C': case 'c': return 'G';
        case 'G': case 'g': return 'C';
        case 'T': case 't': return 'A';
        default: return 'N';
    }
}

// One wave per chunk: the bases of its positions (chunks past the device's chunk count -- launched for the host's bound -- count nothing).
__global__ void __launch_bounds__(256) k_chunk_bases(const uint64_t *offsets, const uint32_t *nodes, uint64_t n, const uint64_t *chunk_first, const uint32_t *chunk_path,
                                                      uint64_t chunks_cap, Labels L, uint64_t *chunk_bases) {
    const uint64_t c = blockIdx.x * static_cast<uint64_t>(blockDim.x / WAVE) + threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    if (c >= chunks_cap) return;
    if (c >= chunk_first[n]) { if (lane == 0) chunk_bases[c] = 0; return; }
    const uint64_t row = chunk_path[c];
    const uint64_t lo = offsets[row] + (c - chunk_first[row]) * SEQ_CHUNK, end = offsets[row + 1];
    const uint64_t hi = lo + SEQ_CHUNK < end ? lo + SEQ_CHUNK : end;
    uint64_t bases = 0;
    for (uint64_t k0 = lo + 4 * lane; k0 < hi; k0 += 4 * WAVE) {    // four consecutive positions per lane: their loads overlap
        uint32_t node[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) node[i] = k0 + i < hi ? nodes[k0 + i] : 0u;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            if (k0 + i >= hi) continue;
            uint64_t a, b;
            label_of(L, node[i], a, b);
            bases += b - a;
        }
    }
    for (int d = WAVE / 2; d > 0; d >>= 1) bases += __shfl_down(bases, d, WAVE);
    if (lane == 0) chunk_bases[c] = bases;
}

// Bytes of every row: its bases -- from the line cache of the index (u64[2] per path, [1] = summed label lengths of the forward path) or from
// the scan over the chunks -- and the endmarker.  An id past the sequences of the index gives an empty row without endmarker.
__global__ void __launch_bounds__(256) k_row_bytes(const uint64_t *seq_ids, uint64_t n, uint64_t n_sequences, const uint64_t *cache_path, const uint64_t *chunk_first,
                                                    const uint64_t *bases_before, int endmarker, uint64_t *row_len) {
    const uint64_t p = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (p >= n) return;
    const uint64_t seq = seq_ids[p];
    if (seq >= n_sequences) { row_len[p] = 0; return; }
    const uint64_t bases = cache_path ? cache_path[2 * (seq >> 1) + 1] : bases_before[chunk_first[p + 1]] - bases_before[chunk_first[p]];
    row_len[p] = bases + (endmarker >= 0 ? 1u : 0u);
}

// What the workgroup of a chunk starts from: where its node ids and its bytes begin, how many positions it has, where the endmarker of
// its row goes when it is the row's last chunk (~0: nowhere).
struct __attribute__((aligned(16))) SeqPlan {
    uint64_t ids_at, out_at, endmarker_at;
    uint32_t count, reserved;
};
static_assert(sizeof(SeqPlan) == 32, "two 16-byte loads");

__global__ void __launch_bounds__(256) k_plan_bases(const uint64_t *offsets, uint64_t n, const uint64_t *seq_ids, uint64_t n_sequences, const uint64_t *chunk_first,
                                                     const uint32_t *chunk_path, uint64_t chunks_cap, const uint64_t *bases_before, const uint64_t *row_start, int endmarker,
                                                     SeqPlan *plans) {
    const uint64_t c = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (c >= chunks_cap || c >= chunk_first[n]) return;
    const uint64_t row = chunk_path[c];
    const uint64_t lo = offsets[row] + (c - chunk_first[row]) * SEQ_CHUNK, end = offsets[row + 1];
    SeqPlan plan;
    plan.ids_at = lo;
    plan.count = static_cast<uint32_t>((lo + SEQ_CHUNK < end ? lo + SEQ_CHUNK : end) - lo);
    plan.reserved = 0;
    plan.out_at = row_start[row] + (bases_before[c] - bases_before[chunk_first[row]]);
    plan.endmarker_at = (endmarker >= 0 && c + 1 == chunk_first[row + 1] && seq_ids[row] < n_sequences) ? row_start[row + 1] - 1 : ~uint64_t(0);
    plans[c] = plan;
}

// 16 bytes from any byte address of the labels: five aligned dwords and a byte shift
__device__ __forceinline__ void load16(const uint8_t *bytes, uint64_t at, uint32_t w[4]) {
    const uint32_t *d = reinterpret_cast<const uint32_t *>(bytes + (at & ~uint64_t(3)));
    const uint32_t sh = static_cast<uint32_t>(at & 3u);
    uint32_t r[5];
#pragma unroll
    for (int k = 0; k < 5; k++) r[k] = d[k];
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = __builtin_amdgcn_alignbyte(r[k + 1], r[k], sh);
}

// One workgroup per chunk (see the top of the file).  The bytes of a batch of BATCH positions lie at out[plan.out_at + cursor ...]; unit u of
// the batch is the aligned 16 bytes at (that address rounded down to 16) + 16 u.  Units wholly inside the batch's range leave as one 16-byte
// store, the first and the last -- where the range does not fill them -- byte by byte (the neighbouring bytes belong to other chunks).
__global__ void __launch_bounds__(BASES_THREADS) k_bases(const uint32_t *nodes, uint64_t n, const uint64_t *chunk_first, const SeqPlan *plans, Labels L, int endmarker,
                                                         uint8_t *out) {
    using BlockScan = hipcub::BlockScan<uint32_t, BASES_THREADS, hipcub::BLOCK_SCAN_WARP_SCANS>;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    __shared__ typename BlockScan::TempStorage scan_storage;
    __shared__ uint64_t src[BATCH];                 // first label byte of every node of the batch | REVERSE_BIT
    __shared__ uint32_t place[BATCH + 1];           // where its bases start in the batch's bytes; place[BATCH] = the batch's bytes
    __shared__ uint8_t table[256];                  // support::COMPLEMENT
    if (blockIdx.x >= chunk_first[n]) return;       // (launched for the host's upper bound of the chunk count)
    const uint32_t t = threadIdx.x;
    const SeqPlan plan = plans[blockIdx.x];
    table[t] = complement(t);
    if (t == 0 && plan.endmarker_at != ~uint64_t(0)) out[plan.endmarker_at] = static_cast<uint8_t>(endmarker);
    const uint32_t *const ids = nodes + plan.ids_at;
    uint8_t *const base = out + plan.out_at;
    uint64_t cursor = 0;
    for (uint32_t b0 = 0; b0 < plan.count; b0 += BATCH) {
        const uint32_t cnt = plan.count - b0 < BATCH ? plan.count - b0 : BATCH;
        uint32_t node[PER_THREAD], len[PER_THREAD], sum = 0;
        uint64_t from[PER_THREAD];
#pragma unroll
        for (uint32_t i = 0; i < PER_THREAD; i++) { const uint32_t k = PER_THREAD * t + i; node[i] = k < cnt ? ids[b0 + k] : 0u; }
#pragma unroll
        for (uint32_t i = 0; i < PER_THREAD; i++) {
            uint64_t a = 0, b = 0;
            if (PER_THREAD * t + i < cnt) label_of(L, node[i], a, b);
            len[i] = static_cast<uint32_t>(b - a);
            from[i] = a | ((node[i] & 1u) ? REVERSE_BIT : 0);
            sum += len[i];
        }
        uint32_t pos, total;
        BlockScan(scan_storage).ExclusiveSum(sum, pos, total);
#pragma unroll
        for (uint32_t i = 0; i < PER_THREAD; i++) { place[PER_THREAD * t + i] = pos; src[PER_THREAD * t + i] = from[i]; pos += len[i]; }
        if (t == 0) place[BATCH] = total;
        __syncthreads();
        uint8_t *const to = base + cursor;
        const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(to) & 15u), end = mis + total;
        uint8_t *const aligned = to - mis;
        for (uint32_t u0 = 16 * t; u0 < end; u0 += 16 * BASES_THREADS) {
            const uint32_t first = (u0 > mis ? u0 : mis) - mis;       // the unit's first byte in batch coordinates
            uint32_t lo = 0, hi = cnt;                                 // the last node that starts at or before it (it has bases: see below)
            while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if (place[mid] <= first) lo = mid; else hi = mid; }
            // (a node of zero bases at lo would have place[lo + 1] == place[lo] <= first with lo + 1 < cnt, or lo + 1 == cnt and first >= total)
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            const bool full = u0 >= mis && u0 + 16 <= end;
            if (full && place[lo + 1] >= first + 16) {                  // the unit lies inside one node
                const uint64_t s = src[lo], at = s & ~REVERSE_BIT;
                if (!(s & REVERSE_BIT)) {
                    load16(L.bytes, at + (first - place[lo]), w);
                } else {
                    uint32_t r[4];
                    load16(L.bytes, at + (place[lo + 1] - first) - 16, r);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const uint32_t v = r[3 - k];
                        w[k] = static_cast<uint32_t>(table[v >> 24]) | (static_cast<uint32_t>(table[(v >> 16) & 255u]) << 8) |
                               (static_cast<uint32_t>(table[(v >> 8) & 255u]) << 16) | (static_cast<uint32_t>(table[v & 255u]) << 24);
                    }
                }
            } else {
                uint32_t k = lo;
#pragma unroll
                for (uint32_t j = 0; j < 16; j++) {
                    if (u0 + j < mis || u0 + j >= end) continue;
                    const uint32_t b = u0 + j - mis;
                    while (place[k + 1] <= b) k++;
                    const uint64_t s = src[k], at = s & ~REVERSE_BIT;
                    const uint32_t off = b - place[k];
                    const uint32_t c = (s & REVERSE_BIT) ? table[L.bytes[at + (place[k + 1] - place[k]) - 1 - off]] : L.bytes[at + off];
                    w[j / 4] |= c << (8 * (j % 4));
                }
            }
            if (full) {
                __builtin_nontemporal_store(u32x4{w[0], w[1], w[2], w[3]}, reinterpret_cast<u32x4 *>(aligned + u0));
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 16; j++)
                    if (u0 + j >= mis && u0 + j < end) aligned[u0 + j] = static_cast<uint8_t>(w[j / 4] >> (8 * (j % 4)));
            }
        }
        cursor += total;
        __syncthreads();
    }
}

}  // namespace

namespace gbwt_hip {

Labels labels_of(const gbwt_hip_index *ix) {
    return Labels{ix->labels.bytes.as<uint8_t>(), ix->labels.off.as<uint64_t>(), static_cast<uint64_t>(ix->host.sequences_labels.size()),
                  static_cast<uint32_t>(ix->host.alphabet_offset + 1)};
}

// The node labels in HBM, made once per handle by the first request for bases (any thread, any workspace).  A failure marks nothing:
// the next request tries again.
void ensure_labels(const gbwt_hip_index *ix) {
    ix->labels.built.ensure([ix]() {
        const Strings &s = ix->host.sequences_labels;
        HIP_CHECK(hipSetDevice(ix->device));
        const uint64_t bytes = s.bytes.size(), offsets = s.offsets.size();
        ix->labels.bytes.reserve(bytes + LABEL_PAD);
        ix->labels.off.reserve(offsets * sizeof(uint64_t));
        if (bytes) HIP_CHECK(hipMemcpy(ix->labels.bytes.ptr, s.bytes.data(), bytes, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(ix->labels.bytes.as<uint8_t>() + bytes, 0, LABEL_PAD));
        HIP_CHECK(hipMemcpy(ix->labels.off.ptr, s.offsets.data(), offsets * sizeof(uint64_t), hipMemcpyHostToDevice));
        uint64_t longest = 0;
        for (uint64_t k = 0; k + 1 < offsets; k++) longest = std::max<uint64_t>(longest, s.offsets[k + 1] - s.offsets[k]);
        ix->labels.max_len = longest;
    });
}

void require_bases_capable(const gbwt_hip_index *ix) {
    if (!ix->host.is_gbz) throw InvalidData("bases need a GBZ (node labels), this handle holds a bare GBWT");
    if (!(ix->caps & GBWT_HIP_OPEN_EXTRACT)) throw InvalidData("the handle was not opened for extraction (GBWT_HIP_OPEN_EXTRACT)");
}

}  // namespace gbwt_hip

// k_bases counts the bytes of a batch of BATCH positions, the slack of its units included, in 32 bits (after ensure_labels)
static const char *const LABELS_TOO_LONG = "node labels too long for the bases kernel (32-bit offsets inside a batch of 1 024 positions)";
static bool labels_fit_a_batch(const gbwt_hip_index *ix) {
    return static_cast<uint64_t>(BATCH) * ix->labels.max_len + 16 * BASES_THREADS + 16 <= 0xFFFFFFFFull;
}

// The bases of a batch of paths, computed ONCE into device memory (text buffer of `slot`: ws->bases.text or text2; row k at
// [offsets[k], offsets[k + 1]) of ws->bases.offsets).  The request is remembered in the workspace: the fill call after a size query, and the
// copy-out of gbwt_hip_path_sequences after gbwt_hip_path_sequences_device, find the bases there.
static gbwt_hip_status sequences_compute(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int reverse, int endmarker,
                                         int slot = 0) {
    if (!ix || !ws || ws->index != ix) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    if (n && !path_ids) return fail(GBWT_HIP_BAD_ARGUMENT, "null path_ids");
    if (endmarker < -1 || endmarker > 255) return fail(GBWT_HIP_BAD_ARGUMENT, "endmarker must be -1 (none) or a byte value 0..255");
    reverse = reverse ? 1 : 0;
    if (ws->bases.memo.matches({{path_ids, n * sizeof(uint64_t)}}, {reverse, endmarker, slot})) return GBWT_HIP_OK;
    ws->bases.memo.drop();
    ws->bases.timed = false;
    try {
        require_bases_capable(ix);
        const HostIndex &h = ix->host;
        HIP_CHECK(hipSetDevice(ix->device));
        hipStream_t s = ws->stream;
        ws->bases.offsets.reserve((n + 1) * sizeof(uint64_t));
        ws->bases.total = 0;
        if (n == 0) {
            HIP_CHECK(hipMemsetAsync(ws->bases.offsets.ptr, 0, sizeof(uint64_t), s));
            HIP_CHECK(hipStreamSynchronize(s));
            ws->bases.memo.store({{nullptr, 0}}, {reverse, endmarker, slot});
            return GBWT_HIP_OK;
        }
        ensure_labels(ix);
        if (!labels_fit_a_batch(ix)) return fail(GBWT_HIP_UNSUPPORTED, LABELS_TOO_LONG);
        // 1. the rows: GBZ::path(id, orientation) = sequence 2 id + orientation (support::encode_path); an id whose sequence does not exist
        // walks nothing and gets an empty row (as in gbwt_hip_extract_paths)
        std::vector<uint64_t> seq_ids(n);
        bool cacheable = !reverse && ix->lc_state == 1;
        for (uint64_t k = 0; k < n; k++) {
            seq_ids[k] = path_ids[k] < (~uint64_t(0)) / 2 ? 2 * path_ids[k] + static_cast<uint64_t>(reverse) : ~uint64_t(0);
            if (seq_ids[k] < h.sequences && path_ids[k] >= h.path_names.size()) cacheable = false;   // (the line cache has the paths of the metadata)
        }
        gbwt_hip_paths paths{};
        const gbwt_hip_status st = gbwt_hip_extract_device(ix, ws, seq_ids.data(), n, &paths);
        if (st != GBWT_HIP_OK) return st;
        ws->bases.ev.ensure();
        ws->extract.pinned_words.ensure();
        HIP_CHECK(hipEventRecord(ws->bases.ev[0], s));
        const uint64_t *d_seq_ids = ws->extract.seq_ids.as<uint64_t>();         // (the extraction has left the ids on the device)
        // 2. sizes.  Chunks of SEQ_CHUNK positions (at least one per row, at most len / SEQ_CHUNK + 1): launches and scans run over that bound.
        const uint64_t chunks_cap = paths.total / SEQ_CHUNK + n;
        if (chunks_cap > 0x7FFFFFFFull) return fail(GBWT_HIP_UNSUPPORTED, "too many chunks in one batch: ask for fewer paths per call");
        const size_t tb = scan_temp_bytes(std::max(n, chunks_cap) + 1);
        ws->scratch.a.reserve(n * sizeof(uint64_t));
        ws->scratch.chunk_first.reserve(2 * (n + 1) * sizeof(uint64_t));
        ws->scratch.chunks.reserve((2 * chunks_cap + 1) * sizeof(uint64_t) + (chunks_cap + 1) * sizeof(uint32_t));
        ws->scratch.plan.reserve(chunks_cap * sizeof(SeqPlan));
        ws->scratch.scan_temp.reserve(std::max<size_t>(tb, 16));
        uint64_t *d_row_len = ws->scratch.a.as<uint64_t>(), *d_row_start = ws->bases.offsets.as<uint64_t>();
        uint64_t *d_chunk_first = ws->scratch.chunk_first.as<uint64_t>(), *d_chunk_counts = d_chunk_first + (n + 1);
        uint64_t *d_chunk_bases = ws->scratch.chunks.as<uint64_t>(), *d_bases_before = d_chunk_bases + chunks_cap;
        uint32_t *d_chunk_path = reinterpret_cast<uint32_t *>(d_bases_before + (chunks_cap + 1));
        const Labels labels = labels_of(ix);
        const unsigned row_blocks = static_cast<unsigned>((n + 255) / 256), chunk_waves = static_cast<unsigned>((chunks_cap + 3) / 4);
        launch_chunk_plan(paths.d_offsets, n, chunks_cap, d_chunk_counts, d_chunk_first, d_chunk_path, ws->scratch.scan_temp.ptr, tb, s);
        const auto chunk_pass = [&]() {
            hipLaunchKernelGGL(k_chunk_bases, dim3(chunk_waves), dim3(256), 0, s, paths.d_offsets, paths.d_nodes, n, d_chunk_first, d_chunk_path, chunks_cap, labels, d_chunk_bases);
            launch_scan(d_chunk_bases, d_bases_before, chunks_cap, ws->scratch.scan_temp.ptr, tb, s);
        };
        // The host waits once, for the total that sizes the text buffer.  With the line cache the rows are sized without a node read and the
        // total leaves before the pass that places the chunks inside their rows: the host's wait and allocation run under that pass.
        if (!cacheable) chunk_pass();
        hipLaunchKernelGGL(k_row_bytes, dim3(row_blocks), dim3(256), 0, s, d_seq_ids, n, h.sequences, cacheable ? ix->lc_path.as<uint64_t>() : nullptr, d_chunk_first,
                           d_bases_before, endmarker, d_row_len);
        launch_scan(d_row_len, d_row_start, n, ws->scratch.scan_temp.ptr, tb, s);
        HIP_CHECK(hipMemcpyAsync(ws->extract.pinned_words.p, d_row_start + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipEventRecord(ws->bases.ev[1], s));
        if (cacheable) chunk_pass();
        HIP_CHECK(hipEventSynchronize(ws->bases.ev[1]));                      // the one wait of a request
        HIP_CHECK(hipGetLastError());
        const uint64_t total = ws->extract.pinned_words.p[0];
        // 3. the bases
        DeviceBuffer &text = slot == 0 ? ws->bases.text : ws->bases.text2;
        text.reserve(std::max<uint64_t>(total, 16));
        hipLaunchKernelGGL(k_plan_bases, dim3(static_cast<unsigned>((chunks_cap + 255) / 256)), dim3(256), 0, s, paths.d_offsets, n, d_seq_ids, h.sequences, d_chunk_first,
                           d_chunk_path, chunks_cap, d_bases_before, d_row_start, endmarker, ws->scratch.plan.as<SeqPlan>());
        HIP_CHECK(hipEventRecord(ws->bases.ev[1], s));
        hipLaunchKernelGGL(k_bases, dim3(static_cast<unsigned>(chunks_cap)), dim3(BASES_THREADS), 0, s, paths.d_nodes, n, d_chunk_first, ws->scratch.plan.as<SeqPlan>(), labels,
                           endmarker, text.as<uint8_t>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ws->bases.ev[2], s));
        HIP_CHECK(hipStreamSynchronize(s));
        ws->bases.timed = true;
        ws->bases.total = total;
        ws->bases.memo.store({{path_ids, n * sizeof(uint64_t)}}, {reverse, endmarker, slot});
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const HipError &e) {
        return status_of(e);
    }
}

extern "C" {

// gbz-extract's extract_sequence (src/bin/gbz-extract.rs:173-191) for a batch of paths, left in HBM
gbwt_hip_status gbwt_hip_path_sequences_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int reverse, int endmarker,
                                               gbwt_hip_lines *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_lines{nullptr, nullptr, 0, 0};
    const gbwt_hip_status st = sequences_compute(ix, ws, path_ids, n, reverse, endmarker);
    if (st != GBWT_HIP_OK) return st;
    out->d_text = ws->bases.text.as<char>();
    out->d_line_offsets = ws->bases.offsets.as<uint64_t>();
    out->total = ws->bases.total;
    out->n = n;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

// The same copied to host buffers: out_offsets[n + 1] (may be NULL), out[total] (NULL = size query)
gbwt_hip_status gbwt_hip_path_sequences(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int reverse, int endmarker, char *out,
                                        uint64_t *out_offsets, uint64_t capacity, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (!total) return fail(GBWT_HIP_BAD_ARGUMENT, "null total");
    *total = 0;
    const gbwt_hip_status st = sequences_compute(ix, ws, path_ids, n, reverse, endmarker);
    if (st != GBWT_HIP_OK) return st;
    *total = ws->bases.total;
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        if (out_offsets) HIP_CHECK(hipMemcpy(out_offsets, ws->bases.offsets.ptr, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (!out || *total == 0) return GBWT_HIP_OK;
        if (capacity < *total) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the bases");
        copy_to_host(ws, out, ws->bases.text.ptr, *total);
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

// GBZ::sequence / sequence_len (src/gbz.rs:292-305) from the host image
gbwt_hip_status gbwt_hip_node_sequence(const gbwt_hip_index *ix, uint64_t node_id, char *out, uint64_t capacity, uint64_t *len, uint8_t *found) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !len || !found) return fail(GBWT_HIP_BAD_ARGUMENT, "null index / len / found");
    *len = 0; *found = 0;
    const HostIndex &h = ix->host;
    if (!h.is_gbz) return fail(GBWT_HIP_BAD_ARGUMENT, "node labels need a GBZ, this handle holds a bare GBWT");
    if (!node_exists(h, node_id)) return GBWT_HIP_OK;
    const uint64_t s = (2 * node_id - (h.alphabet_offset + 1)) / 2;      // GBZ::graph_node_to_sequence (src/gbz.rs:246-255; has_node: 2 node_id > alphabet_offset)
    if (s >= h.sequences_labels.size()) return GBWT_HIP_OK;
    *found = 1;
    *len = h.sequences_labels.len(s);
    if (!out || *len == 0) return GBWT_HIP_OK;
    if (capacity < *len) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the label");
    std::memcpy(out, h.sequences_labels.bytes.data() + h.sequences_labels.offsets[s], *len);
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_sequences_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *sizes_ms, float *bases_ms) {
    GBWT_HIP_GUARD_BEGIN
    if (!ws || !ws->bases.timed || !ws->extract.timed) return fail(GBWT_HIP_BAD_ARGUMENT, "no timed request for bases on this workspace");
    float a = 0, b = 0, c = 0;
    if (hipEventElapsedTime(&a, ws->extract.ev[0], ws->extract.ev[1]) != hipSuccess || hipEventElapsedTime(&b, ws->bases.ev[0], ws->bases.ev[1]) != hipSuccess ||
        hipEventElapsedTime(&c, ws->bases.ev[1], ws->bases.ev[2]) != hipSuccess)
        return fail(GBWT_HIP_DEVICE_ERROR, "hipEventElapsedTime failed");
    if (walk_ms) *walk_ms = a;
    if (sizes_ms) *sizes_ms = b;
    if (bases_ms) *bases_ms = c;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

// gbz-extract -o path (extract_sequences, src/bin/gbz-extract.rs:266-294): the forward bases of the paths, each with its endmarker, into
// `path`, and one line per path into `path`.names (path_name_as_line, :191-194).  Batches bounded by BYTES (GBWT_HIP_SEQ_BATCH_MIB, read at
// call time, default 1 GiB) are made into two device buffers in turn while a writer thread moves the previous one to the file (batch_writer.hpp).
gbwt_hip_status gbwt_hip_write_sequences(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const char *path, const uint64_t *path_ids, uint64_t n, int endmarker) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !ws || ws->index != ix || !path) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace / path");
    if (endmarker < -1 || endmarker > 255) return fail(GBWT_HIP_BAD_ARGUMENT, "endmarker must be -1 (none) or a byte value 0..255");
    try {
        require_bases_capable(ix);
        const HostIndex &h = ix->host;
        if (!h.has_metadata) return fail(GBWT_HIP_BAD_ARGUMENT, "sequence extraction requires GBWT metadata");
        if (!(h.metadata_flags & 1) || h.path_names.empty()) return fail(GBWT_HIP_BAD_ARGUMENT, "sequence extraction requires path names");
        std::vector<uint64_t> ids;
        if (path_ids) ids.assign(path_ids, path_ids + n);
        else for (uint64_t p = 0; p < h.path_names.size(); p++) ids.push_back(p);
        for (uint64_t p : ids)
            if (p >= h.path_names.size() || 2 * p >= h.sequences) return fail(GBWT_HIP_BAD_ARGUMENT, "path id out of range");
        ensure_labels(ix);                                   // refused before a file is created or emptied
        if (!ids.empty() && !labels_fit_a_batch(ix)) return fail(GBWT_HIP_UNSUPPORTED, LABELS_TOO_LONG);
        uint64_t budget = uint64_t(1) << 30;
        if (const char *v = std::getenv("GBWT_HIP_SEQ_BATCH_MIB")) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10)) << 20;
        // bytes of every path: exact from the line cache of the index (summed label lengths of the forward path); else nodes x the mean label
        // length, twice over; else (no lengths known) batches of a fixed number of paths
        std::vector<uint64_t> est(ids.size(), 0);
        if (ix->lc_state == 1) {
            std::vector<uint64_t> totals(2 * h.path_names.size());
            HIP_CHECK(hipSetDevice(ix->device));
            HIP_CHECK(hipMemcpy(totals.data(), ix->lc_path.ptr, totals.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
            for (size_t k = 0; k < ids.size(); k++) est[k] = totals[2 * ids[k] + 1] + 1;
        } else if (!ix->host_seq_len.empty()) {
            const uint64_t labels = std::max<uint64_t>(h.sequences_labels.size(), 1);
            const uint64_t mean = (h.sequences_labels.bytes.size() + labels - 1) / labels;
            for (size_t k = 0; k < ids.size(); k++) est[k] = 2 * mean * ix->host_seq_len[2 * ids[k]] + 1;
        }
        const uint64_t fallback_batch = 4096;
        PositionalFile file, names;
        file.fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (file.fd < 0) return fail(GBWT_HIP_IO_ERROR, std::string("cannot create ") + path);
        const std::string names_path = std::string(path) + ".names";
        names.fd = ::open(names_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (names.fd < 0) return fail(GBWT_HIP_IO_ERROR, std::string("cannot create ") + names_path);
        // Metadata::sample_name / contig_name fall back to the number (src/gbwt.rs:744-761, 792-809)
        const bool sample_names = (h.metadata_flags & 2) != 0, contig_names = (h.metadata_flags & 4) != 0;
        const auto name = [](std::string &line, const Strings &table, bool has, uint64_t id) {
            if (has && id < table.size()) line.append(reinterpret_cast<const char *>(table.bytes.data()) + table.offsets[id], table.len(id));
            else line += std::to_string(id);
        };
        std::string lines;
        uint64_t names_at = 0;
        BatchWriter writer;
        writer.file = &file; writer.device = ix->device; writer.what = "sequences";
        writer.start();
        int slot = 0;
        gbwt_hip_status st = GBWT_HIP_OK;
        std::vector<uint64_t> offs;
        for (uint64_t b0 = 0; b0 < ids.size();) {
            uint64_t nb = 0, bytes = 0;
            while (b0 + nb < ids.size()) {
                if (nb != 0 && (est[b0 + nb] == 0 ? nb >= fallback_batch : bytes + est[b0 + nb] > budget)) break;
                bytes += est[b0 + nb]; nb++;
            }
            if (!writer.acquire(slot)) { st = GBWT_HIP_IO_ERROR; break; }
            st = sequences_compute(ix, ws, ids.data() + b0, nb, 0, endmarker, slot);
            if (st != GBWT_HIP_OK) break;
            writer.submit((slot == 0 ? ws->bases.text : ws->bases.text2).as<char>(), ws->bases.total, slot);
            offs.resize(nb + 1);
            HIP_CHECK(hipMemcpy(offs.data(), ws->bases.offsets.ptr, (nb + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
            lines.clear();
            for (uint64_t k = 0; k < nb; k++) {
                const uint64_t p = ids[b0 + k];
                const PathName &pn = h.path_names[p];
                lines += std::to_string(p); lines += '\t';
                name(lines, h.sample_names, sample_names, pn.sample); lines += '\t';
                name(lines, h.contig_names, contig_names, pn.contig); lines += '\t';
                lines += std::to_string(pn.phase); lines += '\t';
                lines += std::to_string(pn.fragment); lines += '\t';
                lines += std::to_string(offs[k + 1] - offs[k] - (endmarker >= 0 ? 1 : 0)); lines += '\n';
            }
            if (!names.write_at(lines.data(), lines.size(), names_at)) { st = fail(GBWT_HIP_IO_ERROR, "short write"); break; }
            names_at += lines.size();
            slot ^= 1;
            b0 += nb;
        }
        const gbwt_hip_status wst = writer.finish();
        ws->bases.memo.drop();                               // (both text buffers have been reused)
        if (st == GBWT_HIP_OK && wst != GBWT_HIP_OK) return fail(wst, writer.message);
        if (st != GBWT_HIP_OK) return wst != GBWT_HIP_OK ? fail(wst, writer.message) : st;
        if (file.failed || names.failed) return fail(GBWT_HIP_IO_ERROR, "short write");
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

}  // extern "C"
