// merge_meta.hpp -- the host's part of a merge (host only: no HIP in here; tests/cpp/merge_meta.cpp builds it with the sanitizers):
// the metadata, the tags and the node labels of the index of a's sequences followed by b's.  The contract is in include/gbwt_hip.h,
// "merging".
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

#include "host_index.hpp"

namespace gbwt_hip {

struct MergeRefusal {
    enum Kind { NONE = 0, UNSUPPORTED = 1, INVALID = 2 } kind = NONE;
    std::string what;
    explicit operator bool() const { return kind != NONE; }
};

using TagList = std::vector<std::pair<std::string, std::string>>;

inline const std::string *merge_find_tag(const TagList &tags, const std::string &key) {
    for (const auto &t : tags) if (t.first == key) return &t.second;
    return nullptr;
}

// a's names, then those of b's that are not among them, joined by one space
inline std::string merge_reference_samples(const std::string &a, const std::string &b) {
    std::vector<std::string> names;
    const auto add = [&](const std::string &list) {
        size_t at = 0;
        while (at < list.size()) {
            size_t end = list.find(' ', at);
            if (end == std::string::npos) end = list.size();
            if (end > at) {
                const std::string name = list.substr(at, end - at);
                bool known = false;
                for (const std::string &n : names) known = known || n == name;
                if (!known) names.push_back(name);
            }
            at = end + 1;
        }
    };
    add(a); add(b);
    std::string out;
    for (size_t i = 0; i < names.size(); i++) { if (i) out += ' '; out += names[i]; }
    return out;
}

// a's tags in order, then the keys only b has; reference_samples is the union of both lists (where a has the key, at a's place)
inline TagList merge_tags(const TagList &a, const TagList &b) {
    static const std::string RS = "reference_samples";
    const std::string *rs_a = merge_find_tag(a, RS), *rs_b = merge_find_tag(b, RS);
    const std::string rs = merge_reference_samples(rs_a ? *rs_a : std::string(), rs_b ? *rs_b : std::string());
    TagList out;
    for (const auto &t : a) out.emplace_back(t.first, t.first == RS ? rs : t.second);
    for (const auto &t : b)
        if (!merge_find_tag(a, t.first)) out.emplace_back(t.first, t.first == RS ? rs : t.second);
    return out;
}

// a's names in order, then those of b that a lacks, in b's order; map[i] = the id of b's name i in the result
inline Strings merge_names(const Strings &a, const Strings &b, std::vector<uint32_t> &map) {
    Strings out;
    std::unordered_map<std::string, uint32_t> ids;
    const auto intern = [&](const std::string &s) {
        const auto it = ids.find(s);
        if (it != ids.end()) return it->second;
        const uint32_t id = static_cast<uint32_t>(out.size());
        out.bytes.insert(out.bytes.end(), s.begin(), s.end());
        out.offsets.push_back(out.bytes.size());
        ids.emplace(s, id);
        return id;
    };
    for (size_t i = 0; i < a.size(); i++) (void)intern(a.str(i));
    map.clear();
    for (size_t i = 0; i < b.size(); i++) map.push_back(intern(b.str(i)));
    return out;
}

// The metadata of the merged index into `out` (has_metadata .. generic_phase_on_disk); neither input with metadata: none
inline MergeRefusal merge_metadata(const HostIndex &a, const HostIndex &b, HostIndex &out) {
    MergeRefusal bad;
    out.has_metadata = false;
    if (!a.has_metadata && !b.has_metadata) return bad;
    if (a.has_metadata != b.has_metadata) {
        bad.kind = MergeRefusal::UNSUPPORTED;
        bad.what = std::string("only ") + (a.has_metadata ? "a" : "b") + " has metadata: the paths of the other have no names";
        return bad;
    }
    const auto complete = [](const HostIndex &h) { return (h.metadata_flags & 7u) == 7u || (h.path_names.empty() && h.sequences == 0 && (h.metadata_flags & 6u) == 6u); };
    if (!complete(a) || !complete(b)) {
        bad.kind = MergeRefusal::UNSUPPORTED;
        bad.what = std::string("the metadata of ") + (!complete(a) ? "a" : "b") + " lacks path names, sample names or contig names";
        return bad;
    }
    std::vector<uint32_t> sample_map, contig_map;
    out.sample_names = merge_names(a.sample_names, b.sample_names, sample_map);
    out.contig_names = merge_names(a.contig_names, b.contig_names, contig_map);
    out.path_names = a.path_names;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, bool> seen;
    std::map<std::pair<uint32_t, uint32_t>, bool> haplotypes;
    for (const PathName &p : a.path_names) {
        seen[std::make_tuple(p.sample, p.contig, p.phase, p.fragment)] = true;
        haplotypes[{p.sample, p.phase}] = true;
    }
    for (size_t k = 0; k < b.path_names.size(); k++) {
        PathName p = b.path_names[k];
        if (p.sample >= sample_map.size() || p.contig >= contig_map.size()) {
            bad.kind = MergeRefusal::INVALID;
            bad.what = "path " + std::to_string(k) + " of b names a sample or a contig that b does not have";
            return bad;
        }
        p.sample = sample_map[p.sample]; p.contig = contig_map[p.contig];
        const auto key = std::make_tuple(p.sample, p.contig, p.phase, p.fragment);
        if (seen.count(key)) {
            bad.kind = MergeRefusal::INVALID;
            bad.what = "path " + std::to_string(k) + " of b has the name of an earlier path (sample, contig, haplotype, fragment)";
            return bad;
        }
        seen[key] = true;
        haplotypes[{p.sample, p.phase}] = true;
        out.path_names.push_back(p);
    }
    out.has_metadata = true;
    out.metadata_flags = (out.path_names.empty() ? 0u : 1u) | 2u | 4u;
    out.sample_count = out.sample_names.size(); out.contig_count = out.contig_names.size(); out.haplotype_count = haplotypes.size();
    out.generic_phase_on_disk = a.generic_phase_on_disk;
    return bad;
}

// The graph of two GBZ without translations: the union of the node labels over the merged alphabet [alphabet_offset + 1, alphabet_size)
inline MergeRefusal merge_graph(const HostIndex &a, const HostIndex &b, uint64_t alphabet_offset, uint64_t alphabet_size, HostIndex &out) {
    MergeRefusal bad;
    if (a.has_translation || b.has_translation) {
        bad.kind = MergeRefusal::UNSUPPORTED;
        bad.what = std::string(a.has_translation ? "a" : "b") + " has a node-to-segment translation: merging translations is not supported";
        return bad;
    }
    const uint64_t first_node = alphabet_offset + 1, n = alphabet_size > first_node ? (alphabet_size - first_node) / 2 : 0;
    // label k of the result is node id first_node / 2 + k; in an input it is label (2 id - its first node) / 2
    const auto label_in = [](const HostIndex &h, uint64_t id, uint64_t &lo, uint64_t &hi) {
        const uint64_t first = h.alphabet_offset + 1;
        lo = hi = 0;
        if (2 * id < first) return;
        const uint64_t s = (2 * id - first) / 2;
        if (s >= h.sequences_labels.size()) return;
        lo = h.sequences_labels.offsets[s]; hi = h.sequences_labels.offsets[s + 1];
    };
    Strings labels;
    uint64_t nodes = 0;
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t id = (first_node + 2 * k) / 2;
        uint64_t al, ah, bl, bh;
        label_in(a, id, al, ah); label_in(b, id, bl, bh);
        const uint8_t *pa = a.sequences_labels.bytes.data() + al, *pb = b.sequences_labels.bytes.data() + bl;
        if (ah > al && bh > bl && (ah - al != bh - bl || !std::equal(pa, pa + (ah - al), pb))) {
            bad.kind = MergeRefusal::INVALID;
            bad.what = "node " + std::to_string(id) + " has different labels in a and in b";
            return bad;
        }
        if (ah > al) labels.bytes.insert(labels.bytes.end(), pa, pa + (ah - al));
        else if (bh > bl) labels.bytes.insert(labels.bytes.end(), pb, pb + (bh - bl));
        if (ah > al || bh > bl) nodes++;
        labels.offsets.push_back(labels.bytes.size());
    }
    fill_gfa_graph(out, std::move(labels), nodes);
    return bad;
}

}  // namespace gbwt_hip
