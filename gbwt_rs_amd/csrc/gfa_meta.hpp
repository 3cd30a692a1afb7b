// gfa_meta.hpp -- the host's part of a construction from GFA (host only: no HIP in here; tests/cpp/gfa_meta.cpp builds it with the
// sanitizers): the file, the counts of gbwt_hip_parse_gfa, the metadata from the name fields of the P- and W-lines, the reference
// samples of a header line, and the graph part of the HostIndex.  The contract is in include/gbwt_hip.h, "construction from GFA".
#pragma once

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <string_view>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "host_index.hpp"

namespace gbwt_hip {

struct GfaCounts {
    uint64_t bytes = 0, lines = 0, headers = 0, segments = 0, links = 0, p_lines = 0, w_lines = 0, ignored_lines = 0, steps = 0, label_bytes = 0;
};

// A P- or W-line as the device hands it back: its 0-based line number and the positions of its first tabs (two of a P-line, six of a
// W-line).  Field k lies between tab k - 1 and tab k.
struct GfaPathLine {
    uint64_t line = 0;
    uint32_t walk = 0;
    uint64_t tab[6] = {0, 0, 0, 0, 0, 0};
};

// The name fields of a path line.  P: a = name.  W: a = sample, b = haplotype, c = contig, d = start.
struct GfaPathFields {
    uint64_t line = 0;       // 0-based
    bool walk = false;
    std::string_view a, b, c, d;
};

inline GfaPathFields gfa_path_fields(const char *text, const GfaPathLine &p) {
    const auto field = [&](int k) { return std::string_view(text + p.tab[k - 1] + 1, p.tab[k] - p.tab[k - 1] - 1); };
    GfaPathFields f;
    f.line = p.line; f.walk = p.walk != 0;
    f.a = field(1);
    if (f.walk) { f.b = field(2); f.c = field(3); f.d = field(4); }
    return f;
}

struct GfaMetaRefusal {
    uint64_t line = 0;       // 1-based; 0: none
    std::string what;
    explicit operator bool() const { return line != 0; }
};

// digits only, below `limit`
inline bool gfa_decimal(std::string_view s, uint64_t limit, uint64_t &value) {
    if (s.empty() || s.size() > 19) return false;
    value = 0;
    for (char c : s) {
        if (c < '0' || c > '9') return false;
        value = value * 10 + static_cast<uint64_t>(c - '0');
    }
    return value < limit;
}

// Metadata of the paths, in path order.  Sample names: "_gbwt_ref" first iff there is a P-line, then the W samples by first appearance;
// contig names by first appearance over the paths; a P-line is (_gbwt_ref, name, 0, 0), a W-line (sample, contig, haplotype, start) with
// start "*" = 0; haplotype_count = distinct (sample, phase).  Paths from 0-based line `stop_line` on are not looked at (the device has
// refused a line before them).  The first offending line in FILE order is reported: of two paths with one name, the later one.
inline GfaMetaRefusal assemble_gfa_metadata(const std::vector<GfaPathFields> &paths, uint64_t stop_line, HostIndex &h) {
    GfaMetaRefusal bad;
    const auto refuse = [&](uint64_t line, const std::string &what) {
        if (!bad || line + 1 < bad.line) { bad.line = line + 1; bad.what = what; }
    };
    h.path_names.clear();
    h.sample_names = Strings(); h.contig_names = Strings();
    std::unordered_map<std::string, uint32_t> samples, contigs;
    const auto intern = [](std::unordered_map<std::string, uint32_t> &ids, Strings &names, std::string_view s) {
        const auto it = ids.find(std::string(s));
        if (it != ids.end()) return it->second;
        const uint32_t id = static_cast<uint32_t>(names.size());
        names.bytes.insert(names.bytes.end(), s.begin(), s.end());
        names.offsets.push_back(names.bytes.size());
        ids.emplace(std::string(s), id);
        return id;
    };
    bool generic = false;
    for (const GfaPathFields &p : paths) generic = generic || !p.walk;
    if (generic) intern(samples, h.sample_names, "_gbwt_ref");
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, uint64_t> seen;   // name -> line
    std::map<std::pair<uint32_t, uint32_t>, bool> haplotypes;
    for (const GfaPathFields &p : paths) {
        if (p.line >= stop_line) { h.path_names.push_back(PathName{0, 0, 0, 0}); continue; }
        PathName name{0, 0, 0, 0};
        if (!p.walk) {
            name.contig = intern(contigs, h.contig_names, p.a);
        } else {
            uint64_t hap = 0, start = 0;
            if (!gfa_decimal(p.b, 0xFFFFFFFFull, hap)) { refuse(p.line, "W-line: the haplotype is not a decimal number below 2^32 - 1"); continue; }
            if (p.d != "*" && !gfa_decimal(p.d, uint64_t(1) << 32, start)) { refuse(p.line, "W-line: the start is neither * nor a decimal number below 2^32"); continue; }
            name.sample = intern(samples, h.sample_names, p.a);
            name.contig = intern(contigs, h.contig_names, p.c);
            name.phase = static_cast<uint32_t>(hap); name.fragment = static_cast<uint32_t>(start);
        }
        h.path_names.push_back(name);
        const auto key = std::make_tuple(name.sample, name.contig, name.phase, name.fragment);
        const auto twin = seen.find(key);
        if (twin != seen.end()) refuse(std::max(twin->second, p.line), "two paths with the same name (sample, contig, haplotype, fragment)");
        else seen.emplace(key, p.line);
        haplotypes[{name.sample, name.phase}] = true;
    }
    h.has_metadata = true;
    h.metadata_flags = (paths.empty() ? 0u : 1u) | 2u | 4u;
    h.sample_count = h.sample_names.size(); h.contig_count = h.contig_names.size(); h.haplotype_count = haplotypes.size();
    h.generic_phase_on_disk = true;
    return bad;
}

// The value of the RS:Z: field of a header line
inline bool gfa_reference_samples(std::string_view line, std::string &value) {
    size_t at = 0;
    while (at <= line.size()) {
        size_t end = line.find('\t', at);
        if (end == std::string_view::npos) end = line.size();
        const std::string_view field = line.substr(at, end - at);
        if (field.substr(0, 5) == "RS:Z:") { value = std::string(field.substr(5)); return true; }
        at = end + 1;
    }
    return false;
}

// (the graph of a GBZ without a translation: host_index.hpp, fill_gfa_graph)
// The graph of a GBZ with a translation, as the loader leaves it: one label per node 1 .. mapping_len - 1 (empty where no path goes), the
// names of the segments (empty likewise) and the first node of each
inline void fill_gfa_translated_graph(HostIndex &h, Strings &&labels, uint64_t graph_nodes, Strings &&names, Words &&starts, uint64_t mapping_len) {
    h.is_gbz = true; h.has_translation = true;
    h.graph_nodes = graph_nodes;
    h.sequences_labels = std::move(labels);
    h.segment_names = std::move(names); h.segment_starts = std::move(starts); h.mapping_len = mapping_len;
}

// The counts of a text, without a device and without the checks of a construction (only a carriage return is refused): what
// gbwt_hip_parse_gfa answers.  steps: the orientation marks of the step fields; label_bytes: the sequences of all S-lines.
inline GfaCounts count_gfa_on_host(const char *text, uint64_t len) {
    GfaCounts c;
    c.bytes = len;
    uint64_t at = 0, number = 0;
    while (at < len) {
        const char *nl = static_cast<const char *>(std::memchr(text + at, '\n', len - at));
        const uint64_t end = nl ? static_cast<uint64_t>(nl - text) : len;
        number++;
        if (std::memchr(text + at, '\r', end - at)) throw InvalidData("GFA line " + std::to_string(number) + ": a carriage return");
        if (end > at) {
            c.lines++;
            std::vector<uint64_t> tabs;
            for (uint64_t i = at; i < end && tabs.size() < 7; i++) if (text[i] == '\t') tabs.push_back(i);
            const auto field = [&](size_t k) {      // [begin, end) of field k >= 1
                const uint64_t lo = tabs[k - 1] + 1, hi = k < tabs.size() ? tabs[k] : end;
                return std::make_pair(lo, hi);
            };
            const auto marks = [&](std::pair<uint64_t, uint64_t> f, char x, char y) {
                uint64_t n = 0;
                for (uint64_t i = f.first; i < f.second; i++) n += text[i] == x || text[i] == y;
                return n;
            };
            switch (text[at]) {
                case 'H': c.headers++; break;
                case 'S': c.segments++; if (tabs.size() >= 2) c.label_bytes += field(2).second - field(2).first; break;
                case 'L': c.links++; break;
                case 'P': c.p_lines++; if (tabs.size() >= 2) c.steps += marks(field(2), '+', '-'); break;
                case 'W': c.w_lines++; if (tabs.size() >= 6) c.steps += marks(field(6), '>', '<'); break;
                default: c.ignored_lines++;
            }
        }
        at = end + 1;
    }
    return c;
}

// A file, mapped (read-only) for as long as the object lives
class GfaFile {
public:
    explicit GfaFile(const std::string &path) {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) throw IoError("cannot open " + path);
        struct stat st;
        if (::fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { ::close(fd); throw IoError("cannot read " + path); }
        len_ = static_cast<uint64_t>(st.st_size);
        if (len_) {
            void *p = ::mmap(nullptr, len_, PROT_READ, MAP_PRIVATE, fd, 0);
            if (p == MAP_FAILED) { ::close(fd); throw IoError("cannot map " + path); }
            data_ = static_cast<const char *>(p);
        }
        ::close(fd);
    }
    ~GfaFile() { if (data_) ::munmap(const_cast<char *>(data_), len_); }
    GfaFile(const GfaFile &) = delete;
    GfaFile &operator=(const GfaFile &) = delete;
    const char *data() const { return data_; }
    uint64_t size() const { return len_; }

private:
    const char *data_ = nullptr;
    uint64_t len_ = 0;
};

}  // namespace gbwt_hip
