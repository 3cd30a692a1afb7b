// gfa_host.cpp -- the host's side of the GFA text, plain C++ over the host image of the index (HostIndex): GBZ::has_node and the edge list
// of a record read from the record bytes, the node-to-segment translation, the replay of the reference's SegmentPathIter for paths that are
// not concatenations of whole segments, and the H-, S- and L-lines of a whole file (gbwt_hip_write_gfa*).  No HIP: built by the host
// compiler next to host_index.cpp, and run without a GPU by tests/cpp/gfa_host.cpp.
#include "gfa_host.hpp"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>

namespace gbwt_hip {

// Edge list of a record, decoded on the host (Record::decompress_edges, src/bwt.rs:378-395) for the L-lines.
bool host_edges(const HostIndex &h, uint64_t rec, std::vector<std::pair<uint64_t, uint64_t>> &edges) {
    edges.clear();
    if (rec >= h.records()) return false;
    h.ensure_records();
    const uint8_t *p = h.data.data() + h.starts[rec], *end = h.data.data() + h.starts[rec + 1];
    auto varint = [&](uint64_t &v) -> bool {
        v = 0;
        unsigned shift = 0;
        while (p < end) {
            uint8_t b = *p++;
            if (shift < 64) v += static_cast<uint64_t>(b & 0x7F) << shift;
            shift += 7;
            if (!(b & 0x80)) return true;
        }
        return false;
    };
    uint64_t sigma = 0, node = 0;
    if (!varint(sigma) || sigma == 0) return false;
    for (uint64_t e = 0; e < sigma; e++) {
        uint64_t delta, off;
        if (!varint(delta) || !varint(off)) return false;
        node += delta;
        edges.emplace_back(node, off);
    }
    return true;
}

// GBZ::has_node (src/gbz.rs:286-289): the forward GBWT node is in the alphabet and its record is not empty
bool node_exists(const HostIndex &h, uint64_t node_id) {
    const uint64_t node = 2 * node_id, first = h.alphabet_offset + 1;
    if (node < first || node >= h.alphabet_size) return false;
    const uint64_t rec = node - h.alphabet_offset;
    h.ensure_records();
    return rec < h.records() && h.starts[rec + 1] > h.starts[rec] && h.data[h.starts[rec]] != 0;
}

// Graph::segment / node_to_segment (src/graph.rs:172-198)
HostSegment host_segment(const HostIndex &h, uint64_t id) {
    return HostSegment{id, h.segment_starts[id], id + 1 < h.segment_starts.size() ? h.segment_starts[id + 1] : h.mapping_len};
}

HostSegment host_node_to_segment(const HostIndex &h, uint64_t node_id) {
    // SparseVector::predecessor: the last one at or before node_id
    const auto it = std::upper_bound(h.segment_starts.begin(), h.segment_starts.end(), node_id);
    return host_segment(h, static_cast<uint64_t>(it - h.segment_starts.begin()) - 1);
}

// Segment::sequence = labels of nodes start .. end - 1 concatenated (sequences.range(start - 1 .. end - 1))
uint64_t host_segment_seq_len(const HostIndex &h, const HostSegment &s) {
    return h.sequences_labels.offsets[s.end - 1] - h.sequences_labels.offsets[s.start - 1];
}

// SegmentPathIter (src/gbz.rs:1098-1169) over the extracted node ids of one path: the (segment, orientation) tokens up
// to the point where the reference's iterator stops, and the summed segment lengths.
void host_segment_path(const HostIndex &h, const uint32_t *nodes, uint64_t len, std::vector<std::pair<uint64_t, bool>> &tokens, uint64_t &seq_len) {
    tokens.clear();
    seq_len = 0;
    bool have_next = false, next_rev = false;
    uint64_t next_node = 0, seg_start = 0, seg_end = 0;
    for (uint64_t k = 0; k < len; k++) {
        const uint64_t node_id = nodes[k] >> 1;
        const bool rev = (nodes[k] & 1u) != 0;
        if (have_next) {
            if (node_id != next_node || rev != next_rev) return;                  // fail
        } else {
            if (!node_exists(h, node_id) || node_id >= h.mapping_len || node_id < h.segment_starts[0]) return;   // node_to_segment -> None
            const HostSegment s = host_node_to_segment(h, node_id);
            tokens.emplace_back(s.id, rev);
            seq_len += host_segment_seq_len(h, s);
            seg_start = s.start; seg_end = s.end;
            next_node = rev ? seg_end - 1 : seg_start; next_rev = rev; have_next = true;   // visit()
        }
        if (!next_rev) { if (next_node + 1 < seg_end) next_node++; else have_next = false; }   // advance()
        else { if (next_node > seg_start) next_node--; else have_next = false; }
    }
}

namespace {

// The text of a phase (the S-lines, then the L-lines: the order of the file), made range by range on a few threads.  A range's place in
// the file is behind the ranges before it, so a thread that has its text waits for its turn to take the next stretch of the file (a
// counter, no I/O under it) and then writes it on its own.  At most `threads` ranges of text exist at a time.
struct GraphLineRanges {
    const HostIndex &h;
    PositionalFile &file;
    uint64_t cursor = 0;                   // next free byte of the file
    GraphLineRanges(const HostIndex &index, PositionalFile &f) : h(index), file(f) {}
    std::mutex turn_lock;
    std::condition_variable turn_cv;
    uint64_t turn = 0;                     // the range whose text goes next

    template <class Make>
    void phase(uint64_t items, uint64_t per_range, unsigned threads, Make make) {
        const uint64_t ranges = (items + per_range - 1) / per_range;
        std::atomic<uint64_t> next{0};
        turn = 0;
        auto work = [&]() {
            std::string text;
            for (uint64_t r = next++; r < ranges; r = next++) {
                text.clear();
                make(r * per_range, std::min(items, (r + 1) * per_range), text);
                uint64_t at;
                {
                    std::unique_lock<std::mutex> lock(turn_lock);
                    turn_cv.wait(lock, [&] { return turn == r; });
                    at = cursor; cursor += text.size(); turn = r + 1;
                }
                turn_cv.notify_all();
                (void)file.write_at(text.data(), text.size(), at);
            }
        };
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < threads; t++) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
    }
};

void append_number(std::string &text, uint64_t v) {
    char digits[24];
    int len = 0;
    do { digits[len++] = static_cast<char>('0' + v % 10); v /= 10; } while (v != 0);
    while (len > 0) text.push_back(digits[--len]);
}

}  // namespace

uint64_t host_graph_lines(const HostIndex &h, bool translated, PositionalFile &file) {
    GraphLineRanges out(h, file);
    {   // header (write_gfa_header, src/bin/gbunzip.rs:193-203)
        std::string head;
        if (const std::string *rs = h.tag("reference_samples")) head = "H\tVN:Z:1.1\tRS:Z:" + *rs + "\n";
        else head = "H\tVN:Z:1.1\n";
        (void)file.write_at(head.data(), head.size(), 0);
        out.cursor = head.size();
    }
    // segments + links over the real nodes (write_segments / write_links, src/bin/gbunzip.rs:230-317)
    const uint64_t first = h.alphabet_offset + 1, potential = h.sequences_labels.size();
    h.ensure_records();                                            // the graph lines read the host's image of the records (made now if this is its first use)
    auto real = [&](uint64_t seq) {
        const uint64_t rec = 2 * seq + first - h.alphabet_offset;
        return rec < h.records() && h.starts[rec + 1] > h.starts[rec] && h.data[h.starts[rec]] != 0;
    };
    const unsigned threads = potential >= (uint64_t(1) << 18) ? std::max(1u, std::min(8u, std::thread::hardware_concurrency())) : 1u;
    if (translated) {
        // GBZ::segment_iter keeps the segments whose first node exists (src/gbz.rs:927-929); links go from the last
        // node of the segment in the orientation of travel (segment_successors, src/gbz.rs:402-415) and are named by
        // the segment of the successor; LinkIter ends at a successor without a segment (src/gbz.rs:996-999)
        const uint64_t n_seg = h.segment_starts.size();
        out.phase(n_seg, uint64_t(1) << 15, threads, [&](uint64_t lo, uint64_t hi, std::string &text) {
            for (uint64_t id = lo; id < hi; id++) {
                const HostSegment seg = host_segment(h, id);
                if (!node_exists(h, seg.start)) continue;
                text += "S\t"; text += h.segment_names.str(id); text += "\t";
                text.append(reinterpret_cast<const char *>(h.sequences_labels.bytes.data()) + h.sequences_labels.offsets[seg.start - 1], host_segment_seq_len(h, seg));
                text += "\n";
            }
        });
        out.phase(n_seg, uint64_t(1) << 15, threads, [&](uint64_t lo, uint64_t hi, std::string &text) {
            std::vector<std::pair<uint64_t, uint64_t>> edges;
            for (uint64_t id = lo; id < hi; id++) {
                const HostSegment seg = host_segment(h, id);
                if (!node_exists(h, seg.start)) continue;
                const std::string name = h.segment_names.str(id);
                for (int rev = 0; rev < 2; rev++) {
                    const uint64_t node_id = rev ? seg.start : seg.end - 1;
                    if (!node_exists(h, node_id) || !host_edges(h, 2 * node_id + rev - h.alphabet_offset, edges)) continue;
                    for (auto &e : edges) {
                        if (e.first == 0) continue;                   // EdgeIter skips the ENDMARKER edge (src/gbz.rs:833)
                        const uint64_t succ = e.first / 2;
                        const bool succ_rev = (e.first & 1) != 0;
                        if (!node_exists(h, succ) || succ >= h.mapping_len || succ < h.segment_starts[0]) break;
                        const HostSegment to = host_node_to_segment(h, succ);
                        const bool canonical = rev ? (to.id > id || (to.id == id && !succ_rev)) : (to.id >= id);
                        if (!canonical) continue;
                        text += "L\t" + name + (rev ? "\t-\t" : "\t+\t") + h.segment_names.str(to.id) + (succ_rev ? "\t-\t*\n" : "\t+\t*\n");
                    }
                }
            }
        });
        return out.cursor;
    }
    out.phase(potential, uint64_t(1) << 16, threads, [&](uint64_t lo, uint64_t hi, std::string &text) {
        for (uint64_t seq = lo; seq < hi; seq++) {
            if (!real(seq)) continue;
            text += "S\t"; append_number(text, (2 * seq + first) / 2); text.push_back('\t');
            text.append(reinterpret_cast<const char *>(h.sequences_labels.bytes.data()) + h.sequences_labels.offsets[seq], h.sequences_labels.len(seq));
            text.push_back('\n');
        }
    });
    out.phase(potential, uint64_t(1) << 16, threads, [&](uint64_t lo, uint64_t hi, std::string &text) {
        std::vector<std::pair<uint64_t, uint64_t>> edges;
        for (uint64_t seq = lo; seq < hi; seq++) {
            if (!real(seq)) continue;
            const uint64_t node_id = (2 * seq + first) / 2;
            for (int rev = 0; rev < 2; rev++) {
                if (!host_edges(h, 2 * node_id + rev - h.alphabet_offset, edges)) continue;
                for (auto &e : edges) {
                    if (e.first == 0) continue;                       // EdgeIter skips the ENDMARKER edge (src/gbz.rs:833)
                    const uint64_t succ = e.first / 2;
                    const bool succ_rev = (e.first & 1) != 0;
                    const bool canonical = rev ? (succ > node_id || (succ == node_id && !succ_rev)) : (succ >= node_id);
                    if (!canonical) continue;
                    text += "L\t"; append_number(text, node_id); text += rev ? "\t-\t" : "\t+\t"; append_number(text, succ); text += succ_rev ? "\t-\t*\n" : "\t+\t*\n";
                }
            }
        }
    });
    return out.cursor;
}

}  // namespace gbwt_hip
