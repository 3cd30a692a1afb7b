// remove_meta.hpp -- the host's part of a removal (host only: no HIP in here; tests/cpp/remove_meta.cpp builds it with the sanitizers):
// the check of the path ids, and the metadata, the tags and the node labels of an index without some of its paths.  The contract is in
// include/gbwt_hip.h, "removal".
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "host_index.hpp"
#include "merge_meta.hpp"

namespace gbwt_hip {

// Path ids below `paths`, each once; else false and the message, which names the first offending id
inline bool remove_check_ids(const uint64_t *ids, uint64_t n, uint64_t paths, std::string &what) {
    std::unordered_set<uint64_t> seen;
    for (uint64_t k = 0; k < n; k++) {
        if (ids[k] >= paths) { what = "path id " + std::to_string(ids[k]) + " is not below the number of paths (" + std::to_string(paths) + ")"; return false; }
        if (!seen.insert(ids[k]).second) { what = "path id " + std::to_string(ids[k]) + " appears twice"; return false; }
    }
    return true;
}

// The metadata without the paths with gone[path] set into `out` (has_metadata .. generic_phase_on_disk): the names of the other paths,
// the sample and contig names they use in their old order, the ids remapped
inline MergeRefusal remove_metadata(const HostIndex &in, const std::vector<uint8_t> &gone, HostIndex &out) {
    MergeRefusal bad;
    out.has_metadata = false;
    if (!in.has_metadata) return bad;
    const bool complete = (in.metadata_flags & 7u) == 7u || (in.path_names.empty() && in.sequences == 0 && (in.metadata_flags & 6u) == 6u);
    if (!complete) {
        bad.kind = MergeRefusal::UNSUPPORTED;
        bad.what = "the metadata lacks path names, sample names or contig names";
        return bad;
    }
    std::vector<uint8_t> sample_used(in.sample_names.size(), 0), contig_used(in.contig_names.size(), 0);
    for (size_t k = 0; k < in.path_names.size(); k++) {
        if (k < gone.size() && gone[k]) continue;
        const PathName &p = in.path_names[k];
        if (p.sample >= sample_used.size() || p.contig >= contig_used.size()) {
            bad.kind = MergeRefusal::INVALID;
            bad.what = "path " + std::to_string(k) + " names a sample or a contig that the index does not have";
            return bad;
        }
        sample_used[p.sample] = 1; contig_used[p.contig] = 1;
    }
    const auto keep = [](const Strings &names, const std::vector<uint8_t> &used, std::vector<uint32_t> &map) {
        Strings kept;
        map.assign(names.size(), 0);
        for (size_t i = 0; i < names.size(); i++) {
            if (!used[i]) continue;
            map[i] = static_cast<uint32_t>(kept.size());
            kept.bytes.insert(kept.bytes.end(), names.bytes.begin() + names.offsets[i], names.bytes.begin() + names.offsets[i + 1]);
            kept.offsets.push_back(kept.bytes.size());
        }
        return kept;
    };
    std::vector<uint32_t> sample_map, contig_map;
    out.sample_names = keep(in.sample_names, sample_used, sample_map);
    out.contig_names = keep(in.contig_names, contig_used, contig_map);
    out.path_names.clear();
    std::map<std::pair<uint32_t, uint32_t>, bool> haplotypes;
    for (size_t k = 0; k < in.path_names.size(); k++) {
        if (k < gone.size() && gone[k]) continue;
        PathName p = in.path_names[k];
        p.sample = sample_map[p.sample]; p.contig = contig_map[p.contig];
        haplotypes[{p.sample, p.phase}] = true;
        out.path_names.push_back(p);
    }
    out.has_metadata = true;
    out.metadata_flags = (out.path_names.empty() ? 0u : 1u) | 2u | 4u;
    out.sample_count = out.sample_names.size(); out.contig_count = out.contig_names.size(); out.haplotype_count = haplotypes.size();
    out.generic_phase_on_disk = in.generic_phase_on_disk;
    return bad;
}

// The tags, copied; reference_samples loses the names that were samples of `before` and are none of `after`, and goes when none is left
inline TagList remove_tags(const TagList &tags, const Strings &before, const Strings &after) {
    static const std::string RS = "reference_samples";
    const auto has = [](const Strings &names, const std::string &name) {
        for (size_t i = 0; i < names.size(); i++)
            if (names.len(i) == name.size() && std::equal(name.begin(), name.end(), names.bytes.begin() + names.offsets[i])) return true;
        return false;
    };
    TagList out;
    for (const auto &t : tags) {
        if (t.first != RS) { out.push_back(t); continue; }
        std::string kept;
        size_t at = 0;
        while (at < t.second.size()) {
            size_t end = t.second.find(' ', at);
            if (end == std::string::npos) end = t.second.size();
            if (end > at) {
                const std::string name = t.second.substr(at, end - at);
                if (!has(before, name) || has(after, name)) { if (!kept.empty()) kept += ' '; kept += name; }
            }
            at = end + 1;
        }
        if (!kept.empty()) out.emplace_back(RS, kept);
    }
    return out;
}

// The graph of a GBZ without a translation over the records of the result (`records`: data, starts with their last entry, alphabet_offset
// and alphabet_size set): the labels of the nodes that are still visited -- the forward record holds an edge --, one per potential node
inline MergeRefusal remove_graph(const HostIndex &in, const HostIndex &records, HostIndex &out) {
    MergeRefusal bad;
    if (in.has_translation) {
        bad.kind = MergeRefusal::UNSUPPORTED;
        bad.what = "the graph has a node-to-segment translation: removing paths from a translated graph is not supported";
        return bad;
    }
    const uint64_t first_node = records.alphabet_offset + 1, n = records.alphabet_size > first_node ? (records.alphabet_size - first_node) / 2 : 0;
    const uint64_t n_records = records.starts.empty() ? 0 : records.starts.size() - 1, in_first = in.alphabet_offset + 1;
    Strings labels;
    uint64_t nodes = 0;
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t id = (first_node + 2 * k) / 2, r = 2 * id - records.alphabet_offset;
        const bool visited = r < n_records && records.starts[r] < records.starts[r + 1] && records.starts[r] < records.data.size() && records.data[records.starts[r]] != 0;
        if (visited && 2 * id >= in_first) {
            const uint64_t s = (2 * id - in_first) / 2;
            if (s < in.sequences_labels.size()) {
                const uint64_t lo = in.sequences_labels.offsets[s], hi = in.sequences_labels.offsets[s + 1];
                labels.bytes.insert(labels.bytes.end(), in.sequences_labels.bytes.begin() + lo, in.sequences_labels.bytes.begin() + hi);
                if (hi > lo) nodes++;
            }
        }
        labels.offsets.push_back(labels.bytes.size());
    }
    fill_gfa_graph(out, std::move(labels), nodes);
    return bad;
}

}  // namespace gbwt_hip
