// gbwt_hip.hpp -- header-only C++17 mirror of the reference's interface for the LF-step path, over the C ABI of
// gbwt_hip.h.  Same names, argument meaning and "not found" behaviour as jltsiren/gbwt-rs (crate gbz 0.5.1):
//   gbwt_hip::GBWT  <->  gbz::GBWT   src/gbwt.rs:108-384  (len, sequences, ..., start, forward, backward, sequence,
//                                                          find, extend, bd_find, extend_forward, extend_backward)
//   gbwt_hip::GBZ   <->  gbz::GBZ    src/gbz.rs:446-544   (paths, path, search_state, follow_forward, follow_backward)
// Option<T> is std::optional<T>; io::ErrorKind::InvalidData and the reference's asserts are gbwt_hip::Error.
// Every method has a batched form (std::vector in, std::vector out) because one device launch per element would
// waste the GPU; the single-element forms exist so that code -- and tests -- written against the reference read the
// same here.  A handle may be shared by threads; each thread needs its own object of this class for the workspace
// (the reference shares &GBZ across rayon workers, src/bin/gbunzip.rs:421-434): use clone_workspace().
#pragma once

#include <algorithm>
#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gbwt_hip.h"

namespace gbwt_hip {

struct Error : std::runtime_error {
    gbwt_hip_status status;
    Error(gbwt_hip_status s, const std::string &what) : std::runtime_error(what), status(s) {}
};

inline void check(gbwt_hip_status s) {
    if (s != GBWT_HIP_OK) throw Error(s, gbwt_hip_last_error());
}

using Pos = gbwt_hip_pos;                        // bwt::Pos
using SearchState = gbwt_hip_state;              // gbwt::SearchState
using BidirectionalState = gbwt_hip_bd_state;    // gbwt::BidirectionalState
enum class Orientation { Forward = 0, Reverse = 1 };   // support::Orientation

constexpr uint64_t ENDMARKER = 0;
inline uint64_t encode_node(uint64_t id, Orientation o) { return 2 * id + static_cast<uint64_t>(o); }        // src/support.rs:160-162
inline uint64_t node_id(uint64_t node) { return node / 2; }                                                  // src/support.rs:166-168
inline Orientation node_orientation(uint64_t node) { return static_cast<Orientation>(node & 1); }            // src/support.rs:172-174
inline uint64_t flip_node(uint64_t node) { return node ^ 1; }                                                // src/support.rs:186-188
inline uint64_t encode_path(uint64_t path_id, Orientation o) { return 2 * path_id + static_cast<uint64_t>(o); }   // src/support.rs:229-231

// CSR result of a batched extraction: row k = nodes[offsets[k] .. offsets[k + 1])
struct Rows {
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> nodes;
    std::vector<uint32_t> row(size_t k) const { return std::vector<uint32_t>(nodes.begin() + offsets[k], nodes.begin() + offsets[k + 1]); }
};

// gbz::ReferencePath (src/gbz.rs:1255-1266): a reference path, its length in bases, and (base offset of a node start, GBWT position of that visit) pairs
struct ReferencePath {
    size_t id, len;
    std::vector<std::pair<size_t, Pos>> positions;
};

class GBWT {
public:
    // serialize::load_from::<GBWT | GBZ>(path)
    // `flags`: what the handle is for (GBWT_HIP_OPEN_EXTRACT | _SEARCH | _GFA): only those structures are built in HBM
    explicit GBWT(const std::string &path, int device = 0, uint32_t flags = GBWT_HIP_OPEN_ALL) {
        gbwt_hip_index *h = nullptr;
        check(gbwt_hip_open_file_flags(path.c_str(), device, flags, &h));
        index_.reset(h, gbwt_hip_close);
        init();
    }
    // an index that is already in memory: raw record stream + record starts + header fields (gbwt_hip_open_records)
    GBWT(const uint8_t *data, uint64_t data_len, const std::vector<uint64_t> &starts, uint64_t alphabet_offset, uint64_t alphabet_size,
         uint64_t sequences, uint64_t size, bool bidirectional, int device = 0, uint32_t flags = GBWT_HIP_OPEN_ALL) {
        gbwt_hip_index *h = nullptr;
        check(gbwt_hip_open_records_flags(data, data_len, starts.data(), starts.size(), alphabet_offset, alphabet_size, sequences, size,
                                          bidirectional ? 1 : 0, device, flags, &h));
        index_.reset(h, gbwt_hip_close);
        init();
    }
    // ---- construction on the device (gbwt_hip.h, "construction"): the index of a set of paths of GBWT-encoded nodes (2 * id + orientation)
    static GBWT from_paths(const std::vector<std::vector<uint64_t>> &paths, bool bidirectional = true, int device = 0, uint32_t flags = GBWT_HIP_OPEN_ALL) {
        std::vector<uint64_t> offsets(1, 0), nodes;
        for (const auto &p : paths) { nodes.insert(nodes.end(), p.begin(), p.end()); offsets.push_back(nodes.size()); }
        gbwt_hip_index *h = nullptr;
        check(gbwt_hip_build_from_paths(offsets.data(), nodes.data(), paths.size(), bidirectional ? 1 : 0, device, flags, &h));
        return GBWT(h);
    }
    // ... of the first n rows of a device-resident extraction (gbwt_hip_extract_device); the rows are only read
    static GBWT from_rows_device(const gbwt_hip_paths &rows, uint64_t n, bool bidirectional = true, int device = 0, uint32_t flags = GBWT_HIP_OPEN_ALL) {
        if (n > rows.n) throw Error(GBWT_HIP_BAD_ARGUMENT, "more rows than the extraction holds");
        gbwt_hip_index *h = nullptr;
        check(gbwt_hip_build_from_rows_device(rows.d_offsets, rows.d_nodes, n, bidirectional ? 1 : 0, device, flags, &h));
        return GBWT(h);
    }
    // the record stream and the dense record starts of the handle (gbwt_hip_records)
    std::pair<std::vector<uint8_t>, std::vector<uint64_t>> records() const {
        uint64_t data_len = 0, n = 0;
        check(gbwt_hip_records(index_.get(), nullptr, 0, &data_len, nullptr, 0, &n));
        std::vector<uint8_t> data(data_len);
        std::vector<uint64_t> starts(n);
        check(gbwt_hip_records(index_.get(), data.data(), data.size(), &data_len, starts.data(), starts.size(), &n));
        return {std::move(data), std::move(starts)};
    }
    // a GBZ handle as a GBZ v1 container, a GBWT handle as a GBWT file
    void save(const std::string &path) const { check(gbwt_hip_save(index_.get(), path.c_str())); }
    gbwt_hip_build_info last_build_info() const {
        gbwt_hip_build_info info{};
        check(gbwt_hip_last_build_info(index_.get(), &info));
        return info;
    }
    // ---- merging on the device (gbwt_hip.h, "merging"): the index of a's sequences followed by b's; a and b are only read
    static GBWT merge(const GBWT &a, const GBWT &b, uint32_t algorithm = GBWT_HIP_MERGE_AUTO, uint32_t flags = GBWT_HIP_OPEN_ALL) { return GBWT(merged_handle(a, b, algorithm, flags)); }
    gbwt_hip_merge_info last_merge_info() const {
        gbwt_hip_merge_info info{};
        check(gbwt_hip_last_merge_info(index_.get(), &info));
        return info;
    }
    // ---- removal on the device (gbwt_hip.h, "removal"): the index without the paths `path_ids`; *this is only read
    GBWT remove_paths(const std::vector<uint64_t> &path_ids, uint32_t algorithm = GBWT_HIP_REMOVE_AUTO, uint32_t flags = GBWT_HIP_OPEN_ALL) const {
        return GBWT(removed_handle(path_ids, algorithm, flags));
    }
    gbwt_hip_remove_info last_remove_info() const {
        gbwt_hip_remove_info info{};
        check(gbwt_hip_last_remove_info(index_.get(), &info));
        return info;
    }
    GBWT clone_workspace() const { GBWT other(*this, 0); return other; }

    // ---- statistics, src/gbwt.rs:108-182
    uint64_t len() const { return stats_.size; }
    bool is_empty() const { return stats_.size == 0; }
    uint64_t sequences() const { return stats_.sequences; }
    uint64_t alphabet_size() const { return stats_.alphabet_size; }
    uint64_t alphabet_offset() const { return stats_.alphabet_offset; }
    uint64_t effective_size() const { return stats_.alphabet_size - stats_.alphabet_offset; }
    uint64_t first_node() const { return stats_.alphabet_offset + 1; }
    bool has_node(uint64_t node) const { return node > stats_.alphabet_offset && node < stats_.alphabet_size; }
    bool is_bidirectional() const { return stats_.bidirectional != 0; }
    bool has_metadata() const { return stats_.has_metadata != 0; }
    const gbwt_hip_stats &stats() const { return stats_; }
    // bytes the index holds on the device and on the host, and what this object's workspace holds (gbwt_hip_memory_usage)
    gbwt_hip_memory memory_usage() const {
        gbwt_hip_memory m{};
        check(gbwt_hip_memory_usage(index_.get(), ws_.get(), &m));
        return m;
    }

    // ---- navigation, src/gbwt.rs:213-261
    std::vector<std::optional<Pos>> start(const std::vector<uint64_t> &ids) const {
        std::vector<Pos> out(ids.size());
        std::vector<uint8_t> valid(ids.size());
        check(gbwt_hip_start(index_.get(), ws_.get(), ids.data(), ids.size(), out.data(), valid.data()));
        return options(out, valid);
    }
    std::optional<Pos> start(uint64_t id) const { return start(std::vector<uint64_t>{id})[0]; }
    std::vector<std::optional<Pos>> forward(const std::vector<Pos> &pos) const { return step(pos, gbwt_hip_forward); }
    std::optional<Pos> forward(Pos pos) const { return forward(std::vector<Pos>{pos})[0]; }
    // panics in the reference when the index is not bidirectional: throws Error here
    std::vector<std::optional<Pos>> backward(const std::vector<Pos> &pos) const { return step(pos, gbwt_hip_backward); }
    std::optional<Pos> backward(Pos pos) const { return backward(std::vector<Pos>{pos})[0]; }
    // GBWT::sequence(id).collect() for every id; an id >= sequences() (no iterator in the reference) gets an empty row.
    // Size query + fill call: the sequences are walked once, the second call finds the rows in the workspace.
    Rows sequences(const std::vector<uint64_t> &ids) const {
        Rows r;
        r.offsets.assign(ids.size() + 1, 0);
        uint64_t total = 0;
        check(gbwt_hip_extract(index_.get(), ws_.get(), ids.data(), ids.size(), r.offsets.data(), nullptr, 0, &total));
        r.nodes.resize(total);
        if (total) check(gbwt_hip_extract(index_.get(), ws_.get(), ids.data(), ids.size(), r.offsets.data(), r.nodes.data(), total, &total));
        return r;
    }
    // Stretch `part` of `parts` of every row (gbwt_hip_extract_part_device): what one of `parts` GPUs walks of a batch they share; the
    // stretches of a row, in order, are sequences(ids).row(k).  Not in the reference: its parallel axis is the path (src/bin/gbunzip.rs:421-434).
    Rows sequences_part(const std::vector<uint64_t> &ids, uint32_t part, uint32_t parts) const {
        Rows r;
        gbwt_hip_paths p{};
        check(gbwt_hip_extract_part_device(index_.get(), ws_.get(), ids.data(), ids.size(), part, parts, &p));
        r.offsets.assign(ids.size() + 1, 0);
        r.nodes.resize(p.total);
        check(gbwt_hip_copy_result(index_.get(), ws_.get(), r.offsets.data(), p.total ? r.nodes.data() : nullptr, p.total));
        return r;
    }
    std::optional<std::vector<uint32_t>> sequence(uint64_t id) const {
        if (id >= sequences()) return std::nullopt;
        return sequences(std::vector<uint64_t>{id}).row(0);
    }

    // ---- search, src/gbwt.rs:269-384
    std::vector<std::optional<SearchState>> find(const std::vector<uint64_t> &nodes) const {
        std::vector<SearchState> out(nodes.size());
        std::vector<uint8_t> valid(nodes.size());
        check(gbwt_hip_find(index_.get(), ws_.get(), nodes.data(), nodes.size(), out.data(), valid.data()));
        return options(out, valid);
    }
    std::optional<SearchState> find(uint64_t node) const { return find(std::vector<uint64_t>{node})[0]; }
    std::vector<std::optional<SearchState>> extend(const std::vector<SearchState> &states, const std::vector<uint64_t> &nodes) const {
        std::vector<SearchState> out(states.size());
        std::vector<uint8_t> valid(states.size());
        check(gbwt_hip_extend(index_.get(), ws_.get(), states.data(), nodes.data(), states.size(), out.data(), valid.data()));
        return options(out, valid);
    }
    std::optional<SearchState> extend(const SearchState &state, uint64_t node) const {
        return extend(std::vector<SearchState>{state}, std::vector<uint64_t>{node})[0];
    }
    std::vector<std::optional<BidirectionalState>> bd_find(const std::vector<uint64_t> &nodes) const {
        std::vector<BidirectionalState> out(nodes.size());
        std::vector<uint8_t> valid(nodes.size());
        check(gbwt_hip_bd_find(index_.get(), ws_.get(), nodes.data(), nodes.size(), out.data(), valid.data()));
        return options(out, valid);
    }
    std::optional<BidirectionalState> bd_find(uint64_t node) const { return bd_find(std::vector<uint64_t>{node})[0]; }
    std::vector<std::optional<BidirectionalState>> extend_forward(const std::vector<BidirectionalState> &states, const std::vector<uint64_t> &nodes) const {
        return bd_extend(states, nodes, gbwt_hip_extend_forward);
    }
    std::optional<BidirectionalState> extend_forward(const BidirectionalState &state, uint64_t node) const {
        return extend_forward(std::vector<BidirectionalState>{state}, std::vector<uint64_t>{node})[0];
    }
    std::vector<std::optional<BidirectionalState>> extend_backward(const std::vector<BidirectionalState> &states, const std::vector<uint64_t> &nodes) const {
        return bd_extend(states, nodes, gbwt_hip_extend_backward);
    }
    std::optional<BidirectionalState> extend_backward(const BidirectionalState &state, uint64_t node) const {
        return extend_backward(std::vector<BidirectionalState>{state}, std::vector<uint64_t>{node})[0];
    }

    // ---- graph topology
    // GBZ::weakly_connected_components (src/gbz.rs:570-598): the node ids of every component, the components in order of their smallest
    // node id, the nodes ascending inside.  Made on the device by the first call on the handle.
    std::vector<std::vector<size_t>> weakly_connected_components() const {
        uint64_t components = 0, nodes = 0;
        check(gbwt_hip_weakly_connected_components(index_.get(), nullptr, 0, nullptr, 0, &components, &nodes));
        std::vector<uint64_t> offsets(components + 1, 0), ids(nodes);
        check(gbwt_hip_weakly_connected_components(index_.get(), offsets.data(), offsets.size(), ids.data(), ids.size(), &components, &nodes));
        std::vector<std::vector<size_t>> out(components);
        for (uint64_t c = 0; c < components; c++) out[c].assign(ids.begin() + offsets[c], ids.begin() + offsets[c + 1]);
        return out;
    }

    // GBZ::node_iter (src/gbz.rs:312-317): the ids of the nodes that exist, ascending
    std::vector<size_t> node_iter() const {
        uint64_t total = 0;
        check(gbwt_hip_node_ids(index_.get(), nullptr, 0, &total));
        std::vector<uint64_t> ids(std::max<uint64_t>(total, 1));
        check(gbwt_hip_node_ids(index_.get(), ids.data(), ids.size(), &total));
        return std::vector<size_t>(ids.begin(), ids.begin() + total);
    }
    // GBZ::successors / predecessors collected (src/gbz.rs:327-353; EdgeIter 819-870): (node id, orientation) pairs, or nullopt
    std::optional<std::vector<std::pair<uint64_t, Orientation>>> successors(uint64_t node_id, Orientation orientation) const {
        return row(gbwt_hip_edges, node_id, orientation, false);
    }
    std::optional<std::vector<std::pair<uint64_t, Orientation>>> predecessors(uint64_t node_id, Orientation orientation) const {
        return row(gbwt_hip_edges, node_id, orientation, true);
    }
    // the batched form: rows of 2 * id + orientation (gbwt_hip_edges)
    struct EdgeRows { std::vector<uint64_t> offsets, edges; std::vector<uint8_t> valid; };
    EdgeRows edges(const std::vector<uint64_t> &node_ids, const std::vector<uint8_t> &orientations, bool predecessors = false) const {
        return rows(gbwt_hip_edges, node_ids, orientations, predecessors);
    }

    // ---- locate: the sequences behind a search state (the C++ GBWT's locate; the reference has no counterpart, include/gbwt_hip.h)
    // the batched form: row k = the ids of the sequences that own offsets start .. end - 1 of states[k] in that order, or (unique) the same
    // ids ascending without duplicates; valid[k] = 0, with an empty row, for a state that is no range of a record (gbwt_hip_locate)
    struct LocatedRows { std::vector<uint64_t> offsets, ids; std::vector<uint8_t> valid; };
    LocatedRows locate(const std::vector<SearchState> &states, bool unique = false) const {
        LocatedRows out;
        out.offsets.assign(states.size() + 1, 0);
        out.valid.assign(states.size(), 0);
        uint64_t total = 0;
        check(gbwt_hip_locate(index_.get(), ws_.get(), states.data(), states.size(), unique ? 1 : 0, out.offsets.data(), nullptr, 0, &total, out.valid.data()));
        out.ids.resize(total);
        if (total) check(gbwt_hip_locate(index_.get(), ws_.get(), states.data(), states.size(), unique ? 1 : 0, out.offsets.data(), out.ids.data(), total, &total, out.valid.data()));
        return out;
    }
    // locate(SearchState): the distinct sequence ids, ascending, or nullopt
    std::optional<std::vector<uint64_t>> locate(const SearchState &state, bool unique = true) const {
        LocatedRows r = locate(std::vector<SearchState>{state}, unique);
        if (!r.valid[0]) return std::nullopt;
        return std::move(r.ids);
    }
    // locate(node, i): the sequence whose visit the position is, or nullopt
    std::vector<std::optional<uint64_t>> locate(const std::vector<Pos> &positions) const {
        std::vector<uint64_t> ids(positions.size());
        std::vector<uint8_t> valid(positions.size());
        check(gbwt_hip_locate_positions(index_.get(), ws_.get(), positions.data(), positions.size(), ids.data(), valid.data()));
        return options(ids, valid);
    }
    std::optional<uint64_t> locate(const Pos &position) const { return locate(std::vector<Pos>{position})[0]; }
    gbwt_hip_locate_info locate_index_info() const {
        gbwt_hip_locate_info info{};
        check(gbwt_hip_locate_index_info(index_.get(), &info));
        return info;
    }

    const gbwt_hip_index *handle() const { return index_.get(); }
    gbwt_hip_workspace *workspace() const { return ws_.get(); }

protected:
    template <class F>
    EdgeRows rows(F fn, const std::vector<uint64_t> &ids, const std::vector<uint8_t> &orientations, bool predecessors) const {
        if (orientations.size() != ids.size()) throw Error(GBWT_HIP_BAD_ARGUMENT, "one orientation per id");
        EdgeRows out;
        out.offsets.assign(ids.size() + 1, 0);
        out.valid.assign(ids.size(), 0);
        uint64_t total = 0;
        check(fn(index_.get(), ws_.get(), ids.data(), orientations.data(), ids.size(), predecessors ? 1 : 0, out.offsets.data(), nullptr, 0, &total, out.valid.data()));
        out.edges.resize(total);
        if (total) check(fn(index_.get(), ws_.get(), ids.data(), orientations.data(), ids.size(), predecessors ? 1 : 0, out.offsets.data(), out.edges.data(), total, &total, out.valid.data()));
        return out;
    }
    template <class F>
    std::optional<std::vector<std::pair<uint64_t, Orientation>>> row(F fn, uint64_t id, Orientation orientation, bool predecessors) const {
        const EdgeRows r = rows(fn, {id}, {static_cast<uint8_t>(orientation == Orientation::Reverse ? 1 : 0)}, predecessors);
        if (!r.valid[0]) return std::nullopt;
        std::vector<std::pair<uint64_t, Orientation>> out;
        for (uint64_t e : r.edges) out.emplace_back(e >> 1, (e & 1) ? Orientation::Reverse : Orientation::Forward);
        return out;
    }
    static gbwt_hip_index *merged_handle(const GBWT &a, const GBWT &b, uint32_t algorithm, uint32_t flags) {
        const gbwt_hip_merge_options options{algorithm, 0, {0, 0}};
        gbwt_hip_index *h = nullptr;
        check(gbwt_hip_merge(a.index_.get(), b.index_.get(), &options, flags, &h));
        return h;
    }
    gbwt_hip_index *removed_handle(const std::vector<uint64_t> &path_ids, uint32_t algorithm, uint32_t flags) const {
        const gbwt_hip_remove_options options{algorithm, 0, {0, 0}};
        gbwt_hip_index *h = nullptr;
        check(gbwt_hip_remove_paths(index_.get(), path_ids.data(), path_ids.size(), &options, flags, &h));
        return h;
    }
    GBWT(const GBWT &other, int) : index_(other.index_), stats_(other.stats_) { make_workspace(); }
    explicit GBWT(gbwt_hip_index *built) { index_.reset(built, gbwt_hip_close); init(); }
    void init() {
        check(gbwt_hip_get_stats(index_.get(), &stats_));
        make_workspace();
    }
    void make_workspace() {
        gbwt_hip_workspace *w = nullptr;
        check(gbwt_hip_workspace_create(index_.get(), &w));
        ws_.reset(w, gbwt_hip_workspace_destroy);
    }
    template <class T>
    static std::vector<std::optional<T>> options(const std::vector<T> &values, const std::vector<uint8_t> &valid) {
        std::vector<std::optional<T>> out(values.size());
        for (size_t k = 0; k < values.size(); k++)
            if (valid[k]) out[k] = values[k];
        return out;
    }
    template <class F>
    std::vector<std::optional<Pos>> step(const std::vector<Pos> &pos, F fn) const {
        std::vector<Pos> out(pos.size());
        std::vector<uint8_t> valid(pos.size());
        check(fn(index_.get(), ws_.get(), pos.data(), pos.size(), out.data(), valid.data()));
        return options(out, valid);
    }
    template <class F>
    std::vector<std::optional<BidirectionalState>> bd_extend(const std::vector<BidirectionalState> &states, const std::vector<uint64_t> &nodes, F fn) const {
        std::vector<BidirectionalState> out(states.size());
        std::vector<uint8_t> valid(states.size());
        check(fn(index_.get(), ws_.get(), states.data(), nodes.data(), states.size(), out.data(), valid.data()));
        return options(out, valid);
    }

    std::shared_ptr<gbwt_hip_index> index_;
    std::shared_ptr<gbwt_hip_workspace> ws_;
    gbwt_hip_stats stats_{};
};

class GBZ : public GBWT {
public:
    explicit GBZ(const std::string &path, int device = 0, uint32_t flags = GBWT_HIP_OPEN_ALL) : GBWT(path, device, flags) {}

private:
    explicit GBZ(gbwt_hip_index *built) : GBWT(built) {}

public:
    // two GBZ: records, metadata, tags and the union of the node labels (gbwt_hip.h, "merging")
    static GBZ merge(const GBZ &a, const GBZ &b, uint32_t algorithm = GBWT_HIP_MERGE_AUTO, uint32_t flags = GBWT_HIP_OPEN_ALL) { return GBZ(merged_handle(a, b, algorithm, flags)); }
    // a GBZ without some of its paths: records, metadata, tags and the labels of the nodes still visited (gbwt_hip.h, "removal")
    GBZ remove_paths(const std::vector<uint64_t> &path_ids, uint32_t algorithm = GBWT_HIP_REMOVE_AUTO, uint32_t flags = GBWT_HIP_OPEN_ALL) const {
        return GBZ(removed_handle(path_ids, algorithm, flags));
    }
    // ---- construction from GFA on the device (gbwt_hip.h, "construction from GFA"): a GBZ like a loaded one, from a file or a text in memory
    static GBZ from_gfa(const std::string &path, int device = 0, uint32_t flags = GBWT_HIP_OPEN_ALL) {
        gbwt_hip_index *h = nullptr;
        check(gbwt_hip_build_from_gfa(path.c_str(), device, flags, &h));
        return GBZ(h);
    }
    static GBZ from_gfa_text(const char *text, uint64_t len, int device = 0, uint32_t flags = GBWT_HIP_OPEN_ALL) {
        gbwt_hip_index *h = nullptr;
        check(gbwt_hip_build_from_gfa_text(text, len, device, flags, &h));
        return GBZ(h);
    }
    // ... with a node-to-segment translation (gbwt_hip.h, gbwt_hip_gfa_options): segment names of any kind, segments chopped to max_node_length
    static GBZ from_gfa(const std::string &path, const gbwt_hip_gfa_options &options, int device = 0, uint32_t flags = GBWT_HIP_OPEN_ALL) {
        gbwt_hip_index *h = nullptr;
        check(gbwt_hip_build_from_gfa_opts(path.c_str(), &options, device, flags, &h));
        return GBZ(h);
    }
    static GBZ from_gfa_text(const char *text, uint64_t len, const gbwt_hip_gfa_options &options, int device = 0, uint32_t flags = GBWT_HIP_OPEN_ALL) {
        gbwt_hip_index *h = nullptr;
        check(gbwt_hip_build_from_gfa_text_opts(text, len, &options, device, flags, &h));
        return GBZ(h);
    }
    gbwt_hip_gfa_translation_info last_gfa_translation_info() const {
        gbwt_hip_gfa_translation_info info{};
        check(gbwt_hip_last_gfa_translation_info(index_.get(), &info));
        return info;
    }
    gbwt_hip_gfa_info last_gfa_info() const {
        gbwt_hip_gfa_info info{};
        check(gbwt_hip_last_gfa_info(index_.get(), &info));
        return info;
    }

    uint64_t paths() const { return sequences() / 2; }   // GBZ::paths, src/gbz.rs:446-452
    // GBZ::path(path_id, orientation).collect(): (node id, orientation) pairs, or nullopt (src/gbz.rs:461-466)
    std::optional<std::vector<std::pair<uint64_t, Orientation>>> path(uint64_t path_id, Orientation orientation) const {
        if (path_id >= paths()) return std::nullopt;
        const Rows r = sequences(std::vector<uint64_t>{encode_path(path_id, orientation)});
        std::vector<std::pair<uint64_t, Orientation>> out;
        for (uint32_t v : r.nodes) out.emplace_back(node_id(v), node_orientation(v));
        return out;
    }
    // GBZ::segment_path(path_id, orientation).collect(): (segment id, orientation) pairs -- the segment as its index in the node-to-segment
    // translation --, or nullopt: no such path, or no translation (src/gbz.rs:477-489; SegmentPathIter 1098-1169)
    std::optional<std::vector<std::pair<uint64_t, Orientation>>> segment_path(uint64_t path_id, Orientation orientation) const {
        if (path_id >= paths() || !stats().has_translation) return std::nullopt;
        const uint64_t id = encode_path(path_id, orientation);
        uint64_t offsets[2] = {0, 0}, total = 0;
        check(gbwt_hip_segment_paths(index_.get(), ws_.get(), &id, 1, offsets, nullptr, 0, &total));
        std::vector<uint64_t> tokens(total);
        if (total) check(gbwt_hip_segment_paths(index_.get(), ws_.get(), &id, 1, offsets, tokens.data(), total, &total));
        std::vector<std::pair<uint64_t, Orientation>> out;
        for (uint64_t t : tokens) out.emplace_back(t >> 1, (t & 1) ? Orientation::Reverse : Orientation::Forward);
        return out;
    }
    // GBZ::has_translation (src/gbz.rs:362-364)
    bool has_translation() const { return stats().has_translation != 0; }
    // GBZ::node_to_segment (src/gbz.rs:370-376): the id of the segment that holds the node, or nullopt
    std::optional<uint64_t> node_to_segment(uint64_t node_id) const {
        uint64_t segment = 0;
        uint8_t valid = 0;
        check(gbwt_hip_node_segments(index_.get(), &node_id, 1, &segment, &valid));
        return valid ? std::optional<uint64_t>(segment) : std::nullopt;
    }
    // GBZ::segment_iter (src/gbz.rs:381-390): the ids of the segments whose first node exists, or nullopt without a translation
    std::optional<std::vector<size_t>> segment_iter() const {
        if (!has_translation()) return std::nullopt;
        uint64_t total = 0;
        check(gbwt_hip_segments(index_.get(), nullptr, 0, &total));
        std::vector<uint64_t> ids(std::max<uint64_t>(total, 1));
        check(gbwt_hip_segments(index_.get(), ids.data(), ids.size(), &total));
        return std::vector<size_t>(ids.begin(), ids.begin() + total);
    }
    // GBZ::segment_successors / segment_predecessors collected (src/gbz.rs:402-440; LinkIter 988-1005): (segment id, orientation) pairs
    std::optional<std::vector<std::pair<uint64_t, Orientation>>> segment_successors(uint64_t segment_id, Orientation orientation) const {
        return row(gbwt_hip_links, segment_id, orientation, false);
    }
    std::optional<std::vector<std::pair<uint64_t, Orientation>>> segment_predecessors(uint64_t segment_id, Orientation orientation) const {
        return row(gbwt_hip_links, segment_id, orientation, true);
    }
    EdgeRows links(const std::vector<uint64_t> &segment_ids, const std::vector<uint8_t> &orientations, bool predecessors = false) const {
        return rows(gbwt_hip_links, segment_ids, orientations, predecessors);
    }
    // the H-, S- and L-lines gbunzip writes (src/bin/gbunzip.rs:193-332), formatted on the device
    std::string graph_lines() const {
        uint64_t total = 0;
        check(gbwt_hip_graph_lines(index_.get(), ws_.get(), nullptr, 0, &total));
        std::string text(total, '\0');
        if (total) check(gbwt_hip_graph_lines(index_.get(), ws_.get(), text.data(), total, &total));
        return text;
    }
    // the same text left in HBM (gbwt_hip_graph_lines_device) and the device times of the last request
    gbwt_hip_graph_text graph_lines_device() const {
        gbwt_hip_graph_text out{};
        check(gbwt_hip_graph_lines_device(index_.get(), ws_.get(), &out));
        return out;
    }
    // GBZ::search_state, src/gbz.rs:508-510
    std::optional<BidirectionalState> search_state(uint64_t id, Orientation orientation) const { return bd_find(encode_node(id, orientation)); }
    // GBZ::follow_forward / follow_backward collected (StateIter, src/gbz.rs:519-544, 1211-1251); nullopt = no iterator
    std::optional<std::vector<BidirectionalState>> follow_forward(const BidirectionalState &state) const { return follow(state, false); }
    std::optional<std::vector<BidirectionalState>> follow_backward(const BidirectionalState &state) const { return follow(state, true); }
    // GBZ::sequence(node_id) (src/gbz.rs:292-298): the node's label, or nullopt for a node that does not exist
    std::optional<std::string> sequence(uint64_t node_id) const {
        uint64_t len = 0;
        uint8_t found = 0;
        check(gbwt_hip_node_sequence(index_.get(), node_id, nullptr, 0, &len, &found));
        if (!found) return std::nullopt;
        std::string label(len, '\0');
        if (len) check(gbwt_hip_node_sequence(index_.get(), node_id, label.data(), len, &len, &found));
        return label;
    }
    // The bases of GBZ::path(path_id, orientation) (gbz-extract's extract_sequence without the endmarker, src/bin/gbz-extract.rs:173-189):
    // labels joined, reverse-oriented ones reverse-complemented; nullopt = no such path
    std::optional<std::string> path_sequence(uint64_t path_id, Orientation orientation) const {
        if (path_id >= paths()) return std::nullopt;
        const int reverse = orientation == Orientation::Reverse ? 1 : 0;
        uint64_t total = 0;
        check(gbwt_hip_path_sequences(index_.get(), ws_.get(), &path_id, 1, reverse, -1, nullptr, nullptr, 0, &total));
        std::string bases(total, '\0');
        if (total) check(gbwt_hip_path_sequences(index_.get(), ws_.get(), &path_id, 1, reverse, -1, bases.data(), nullptr, total, &total));
        return bases;
    }
    // gbz-extract -o path: `path` and `path`.names for all paths (src/bin/gbz-extract.rs:266-294)
    void write_sequences(const std::string &path, int endmarker = 0) const {
        check(gbwt_hip_write_sequences(index_.get(), ws_.get(), path.c_str(), nullptr, 0, endmarker));
    }
    // gbz-extract -m tag-array (src/bin/gbz-extract.rs:408-482): TAG[i] = the graph position of text position sa[i] of the text of these
    // paths (gbwt_hip_tags); `runs` receives the reference's "Tag array runs"
    std::vector<uint64_t> tag_array(const std::vector<uint64_t> &path_ids, const std::vector<uint64_t> &sa, uint64_t *runs = nullptr) const {
        std::vector<uint64_t> tags(sa.size());
        check(gbwt_hip_tags(index_.get(), ws_.get(), path_ids.data(), path_ids.size(), sa.data(), sa.size(), tags.data(), nullptr, runs));
        return tags;
    }
    // the length of that text: the bases of the paths and one endmarker each
    uint64_t text_length(const std::vector<uint64_t> &path_ids) const {
        uint64_t expected_len = 0;
        check(gbwt_hip_tags(index_.get(), ws_.get(), path_ids.data(), path_ids.size(), nullptr, 0, nullptr, &expected_len, nullptr));
        return expected_len;
    }
    // gbz-extract -m tag-array -o base: `base`.names + `base`.sa -> `base`.tags; returns the runs
    uint64_t write_tag_array(const std::string &base, uint64_t sa_skip = 1) const {
        uint64_t runs = 0;
        check(gbwt_hip_write_tag_array(index_.get(), ws_.get(), base.c_str(), sa_skip, &runs));
        return runs;
    }
    // The suffix array of the text of these paths (gbwt_hip_path_suffix_array; the bases of every path and one endmarker each, suffixes
    // compared as unsigned byte strings to the end of the text); `bwt` and `bwt_runs` receive the BWT and its runs
    std::vector<uint64_t> suffix_array(const std::vector<uint64_t> &path_ids, int endmarker = 0, std::vector<uint8_t> *bwt = nullptr, uint64_t *bwt_runs = nullptr) const {
        uint64_t total = 0;
        check(gbwt_hip_path_suffix_array(index_.get(), ws_.get(), path_ids.data(), path_ids.size(), endmarker, nullptr, nullptr, 0, &total, bwt_runs));
        std::vector<uint64_t> sa(total);
        if (bwt) bwt->assign(total, 0);
        if (total) check(gbwt_hip_path_suffix_array(index_.get(), ws_.get(), path_ids.data(), path_ids.size(), endmarker, sa.data(), bwt ? bwt->data() : nullptr, total, &total, bwt_runs));
        return sa;
    }
    // `base`.names (+ `base`) -> `base`.sa and `base`.bwt, what write_tag_array(base) reads; returns the runs of the BWT
    uint64_t write_suffix_array(const std::string &base) const {
        uint64_t runs = 0;
        check(gbwt_hip_write_suffix_array(index_.get(), ws_.get(), base.c_str(), &runs));
        return runs;
    }
    // select_paths of gbz-extract (src/bin/gbz-extract.rs:196-264): every path (nullopt), or the paths of the components in which a path
    // with that contig name starts; throws Error with the reference's messages
    std::vector<size_t> select_paths(const std::optional<std::string> &contig = std::nullopt) const {
        const char *name = contig ? contig->c_str() : nullptr;
        uint64_t total = 0;
        check(gbwt_hip_select_paths(index_.get(), ws_.get(), name, nullptr, 0, &total));
        std::vector<uint64_t> ids(std::max<uint64_t>(total, 1));
        check(gbwt_hip_select_paths(index_.get(), ws_.get(), name, ids.data(), ids.size(), &total));
        return std::vector<size_t>(ids.begin(), ids.begin() + total);
    }
    // gbz-extract -c contig -o path
    void write_sequences(const std::string &path, const std::string &contig, int endmarker) const {
        check(gbwt_hip_write_sequences_contig(index_.get(), ws_.get(), path.c_str(), contig.c_str(), endmarker));
    }
    // GBZ::reference_sample_ids' paths (src/gbz.rs:167-176, 609-629): the ids of the paths of the reference samples, ascending
    std::vector<size_t> reference_paths(bool also_generic = true) const {
        uint64_t count = 0;
        check(gbwt_hip_reference_paths(index_.get(), also_generic ? 1 : 0, nullptr, 0, &count));
        std::vector<uint64_t> ids(std::max<uint64_t>(count, 1));
        check(gbwt_hip_reference_paths(index_.get(), also_generic ? 1 : 0, ids.data(), ids.size(), &count));
        return std::vector<size_t>(ids.begin(), ids.begin() + count);
    }
    // The rule of GBZ::reference_positions for any forward paths, in the order given (gbwt_hip_path_positions)
    std::vector<ReferencePath> path_positions(const std::vector<uint64_t> &path_ids, size_t interval) const {
        uint64_t total = 0;
        std::vector<gbwt_hip_reference_path> rows(std::max<size_t>(path_ids.size(), 1));
        check(gbwt_hip_path_positions(index_.get(), ws_.get(), path_ids.data(), path_ids.size(), interval, rows.data(), nullptr, 0, &total));
        std::vector<gbwt_hip_reference_position> positions(std::max<uint64_t>(total, 1));
        check(gbwt_hip_path_positions(index_.get(), ws_.get(), path_ids.data(), path_ids.size(), interval, nullptr, positions.data(), positions.size(), &total));
        std::vector<ReferencePath> out(path_ids.size());
        for (size_t k = 0; k < path_ids.size(); k++) {
            out[k].id = rows[k].path_id; out[k].len = rows[k].len;
            for (uint64_t q = rows[k].first; q < rows[k].first + rows[k].count; q++) out[k].positions.emplace_back(positions[q].offset, positions[q].pos);
        }
        return out;
    }
    // GBZ::reference_positions(interval, _) (src/gbz.rs:600-657): every reference and generic path, a position about every `interval` bases
    // at the start of a node.  Throws Error without metadata (the reference unwraps it).
    std::vector<ReferencePath> reference_positions(size_t interval) const {
        const std::vector<size_t> ids = reference_paths(true);
        return path_positions(std::vector<uint64_t>(ids.begin(), ids.end()), interval);
    }
    // the lines gbunzip writes for these paths (mode 0 = P-lines, 1 = W-lines) and the whole GFA file
    std::string path_lines(const std::vector<uint64_t> &path_ids, int mode) const {
        uint64_t total = 0;
        check(gbwt_hip_path_lines(index_.get(), ws_.get(), path_ids.data(), path_ids.size(), mode, nullptr, 0, &total));
        std::string text(total, '\0');
        if (total) check(gbwt_hip_path_lines(index_.get(), ws_.get(), path_ids.data(), path_ids.size(), mode, text.data(), total, &total));
        return text;
    }
    // gbunzip --paths MODE (PathMode, src/bin/gbunzip.rs:63-76): GBWT_HIP_PATHS_DEFAULT, _PAN_SN or _REF_ONLY
    void write_gfa(const std::string &path, int path_mode = GBWT_HIP_PATHS_DEFAULT) const {
        check(gbwt_hip_write_gfa_mode(index_.get(), ws_.get(), path.c_str(), path_mode));
    }
    // Metadata::pan_sn_path(path_id) (src/gbwt.rs:709-713) as gbunzip prints it: the name field of the PanSN P-line
    std::string pan_sn_path(uint64_t path_id) const {
        const std::string line = path_lines({path_id}, 2);                 // "P\t<name>\t..."
        const size_t a = line.find('\t'), b = line.find('\t', a + 1);
        return line.substr(a + 1, b - a - 1);
    }

private:
    std::optional<std::vector<BidirectionalState>> follow(const BidirectionalState &state, bool backward) const {
        uint64_t offsets[2] = {0, 0}, total = 0;
        uint8_t valid = 0;
        check(gbwt_hip_follow(index_.get(), ws_.get(), &state, 1, backward ? 1 : 0, offsets, nullptr, 0, &total, &valid));
        if (!valid) return std::nullopt;
        std::vector<BidirectionalState> out(total);
        if (total) check(gbwt_hip_follow(index_.get(), ws_.get(), &state, 1, backward ? 1 : 0, offsets, out.data(), total, &total, &valid));
        return out;
    }
};

// merge(a, b): GBWT::merge for two GBWT, GBZ::merge for two GBZ
template <class Index>
inline Index merge(const Index &a, const Index &b, uint32_t algorithm = GBWT_HIP_MERGE_AUTO, uint32_t flags = GBWT_HIP_OPEN_ALL) { return Index::merge(a, b, algorithm, flags); }

// The suffix array of any bytes, built on `device` (gbwt_hip_suffix_array_text; no index): `bwt` and `bwt_runs` receive the BWT -- with
// `sentinel` in front of suffix 0 -- and its runs
inline std::vector<uint64_t> suffix_array_text(const std::string &text, int sentinel = 0, int device = 0, std::vector<uint8_t> *bwt = nullptr, uint64_t *bwt_runs = nullptr) {
    std::vector<uint64_t> sa(text.size());
    if (bwt) bwt->assign(text.size(), 0);
    check(gbwt_hip_suffix_array_text(device, text.data(), text.size(), sentinel, sa.data(), bwt ? bwt->data() : nullptr, bwt_runs));
    return sa;
}

// The ordered gather of a sharded extraction (one process per GPU; the reference's writer mutex, src/bin/gbunzip.rs:421-434).  Rank 0 makes
// the id (Comm::unique_id), every rank constructs a Comm from it (collective), and after gbwt_hip_extract_device / _path_lines_device on
// each rank's shard gather_rows / gather_lines leave all rows in path order on `root` (device memory of the communicator).
class Comm {
public:
    static gbwt_hip_unique_id unique_id() {
        gbwt_hip_unique_id id{};
        const gbwt_hip_status st = gbwt_hip_comm_unique_id(&id);
        if (st != GBWT_HIP_OK) throw Error(st, gbwt_hip_last_error());
        return id;
    }
    Comm(const gbwt_hip_unique_id &id, int rank, int world, int device) {
        gbwt_hip_comm *c = nullptr;
        const gbwt_hip_status st = gbwt_hip_comm_create(&id, rank, world, device, &c);
        if (st != GBWT_HIP_OK) throw Error(st, gbwt_hip_last_error());
        comm_.reset(c, gbwt_hip_comm_destroy);
    }
    gbwt_hip_comm *get() const { return comm_.get(); }

private:
    std::shared_ptr<gbwt_hip_comm> comm_;
};

}  // namespace gbwt_hip
