// What the host-only programs of this directory (merge_meta.cpp, remove_meta.cpp, adopt_metadata.cpp) share: host images made by hand, and
// their name tables, tags and refusals as text for the lines they print.
#pragma once

#include <string>
#include <vector>

#include "merge_meta.hpp"

using namespace gbwt_hip;

static inline Strings strings(const std::vector<std::string> &names) {
    Strings s;
    for (const std::string &n : names) {
        s.bytes.insert(s.bytes.end(), n.begin(), n.end());
        s.offsets.push_back(s.bytes.size());
    }
    return s;
}

static inline HostIndex with_metadata(const std::vector<std::string> &samples, const std::vector<std::string> &contigs, const std::vector<PathName> &paths) {
    HostIndex h;
    h.bidirectional = true; h.sequences = 2 * paths.size();
    h.has_metadata = true; h.metadata_flags = 7;
    h.sample_names = strings(samples); h.contig_names = strings(contigs); h.path_names = paths;
    h.sample_count = samples.size(); h.contig_count = contigs.size();
    return h;
}

static inline std::string joined(const Strings &s, char sep = ' ') {
    std::string out;
    for (size_t i = 0; i < s.size(); i++) { if (i) out += sep; out += s.str(i); }
    return out;
}

static inline const char *kind(const MergeRefusal &r) { return r.kind == MergeRefusal::NONE ? "none" : r.kind == MergeRefusal::UNSUPPORTED ? "UNSUPPORTED" : "INVALID"; }

static inline std::string tag_line(const TagList &tags) {
    std::string out;
    for (size_t i = 0; i < tags.size(); i++) { if (i) out += '|'; out += tags[i].first + "=" + tags[i].second; }
    return out;
}
