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
// The node labels reach HBM on the first request for bases (ensure_labels), never at open: the upload lives here because the zero bytes
// behind the last label (LABEL_PAD) are what the loads of k_bases may read.  The requests and the C ABI are capi_sequences.hip.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "capi_internal.hpp"
#include "sequences.hpp"

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

// k_bases counts the bytes of a batch of BATCH positions, the slack of its units included, in 32 bits (after ensure_labels)
const char *const LABELS_TOO_LONG = "node labels too long for the bases kernel (32-bit offsets inside a batch of 1 024 positions)";
bool labels_fit_a_batch(const gbwt_hip_index *ix) {
    return static_cast<uint64_t>(BATCH) * ix->labels.max_len + 16 * BASES_THREADS + 16 <= 0xFFFFFFFFull;
}

void launch_chunk_bases(const ChunkedRows &r, const Labels &L, uint64_t *d_chunk_bases, hipStream_t s) {
    hipLaunchKernelGGL(k_chunk_bases, dim3(static_cast<unsigned>((r.chunks_cap + 3) / 4)), dim3(256), 0, s, r.offsets, r.nodes, r.n, r.chunk_first, r.chunk_path, r.chunks_cap, L,
                       d_chunk_bases);
}

void launch_row_bytes(const uint64_t *d_seq_ids, uint64_t n, uint64_t n_sequences, const uint64_t *d_cache_path, const uint64_t *d_chunk_first, const uint64_t *d_bases_before,
                      int endmarker, uint64_t *d_row_len, hipStream_t s) {
    hipLaunchKernelGGL(k_row_bytes, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, d_seq_ids, n, n_sequences, d_cache_path, d_chunk_first, d_bases_before, endmarker,
                       d_row_len);
}

void launch_plan_bases(const ChunkedRows &r, const uint64_t *d_seq_ids, uint64_t n_sequences, const uint64_t *d_bases_before, const uint64_t *d_row_start, int endmarker,
                       SeqPlan *d_plans, hipStream_t s) {
    hipLaunchKernelGGL(k_plan_bases, dim3(static_cast<unsigned>((r.chunks_cap + 255) / 256)), dim3(256), 0, s, r.offsets, r.n, d_seq_ids, n_sequences, r.chunk_first, r.chunk_path,
                       r.chunks_cap, d_bases_before, d_row_start, endmarker, d_plans);
}

void launch_bases(const ChunkedRows &r, const SeqPlan *d_plans, const Labels &L, int endmarker, uint8_t *d_out, hipStream_t s) {
    hipLaunchKernelGGL(k_bases, dim3(static_cast<unsigned>(r.chunks_cap)), dim3(BASES_THREADS), 0, s, r.nodes, r.n, r.chunk_first, d_plans, L, endmarker, d_out);
}

}  // namespace gbwt_hip

