// extract_files.hpp -- the files between gbz-extract's three modes, in one place: `sequences` (capi_sequences.hip) writes `base` and
// `base`.names, the suffix array (capi_suffix_array.hip) and `tag-array` (capi_tags.hip) read them.  The line of a path in `base`.names as it
// is written and as it is read, and the checks every reader makes of what it read.  Plain C++, no HIP (tests/cpp/extract_files.cpp runs it
// without a GPU).  Nothing here sets the error of a call: a failed check comes back as the status and the message the entry point fails with.
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/gbwt_hip.h"

namespace gbwt_hip {

struct FileCheck {
    gbwt_hip_status status = GBWT_HIP_OK;
    std::string message;
    bool ok() const { return status == GBWT_HIP_OK; }
};

// The endmarker argument of the bases and suffix array calls: none, or a byte
constexpr const char *ENDMARKER_RULE = "endmarker must be -1 (none) or a byte value 0..255";
inline bool endmarker_valid(int endmarker) { return endmarker >= -1 && endmarker <= 255; }

// GBZ::path(id, Forward) = sequence 2 id (support::encode_path) is a sequence of the index; no id makes 2 id wrap
inline bool path_exists(uint64_t sequences, uint64_t path_id) { return path_id < (~uint64_t(0)) / 2 && 2 * path_id < sequences; }

// path_name_as_line (src/bin/gbz-extract.rs:191-194): the names of sample and contig as the caller resolved them
inline void append_names_line(std::string &out, uint64_t path_id, const std::string &sample, const std::string &contig, uint64_t phase, uint64_t fragment, uint64_t bases) {
    out += std::to_string(path_id); out += '\t';
    out += sample; out += '\t';
    out += contig; out += '\t';
    out += std::to_string(phase); out += '\t';
    out += std::to_string(fragment); out += '\t';
    out += std::to_string(bases); out += '\n';
}

// 1 to 19 decimal digits (what fits a u64 whatever the digits are)
inline bool parse_names_number(const std::string &field, uint64_t &out) {
    if (field.empty() || field.size() > 19) return false;
    out = 0;
    for (char c : field) { if (c < '0' || c > '9') return false; out = 10 * out + static_cast<uint64_t>(c - '0'); }
    return true;
}

// read_names (src/bin/gbz-extract.rs:296-318): of every line the first tab field = path id, the last tab field = bases
inline FileCheck parse_names(const std::string &text, std::vector<uint64_t> &ids, std::vector<uint64_t> &lens) {
    for (size_t at = 0; at < text.size();) {
        size_t nl = text.find('\n', at);
        if (nl == std::string::npos) nl = text.size();
        std::string line = text.substr(at, nl - at);
        if (!line.empty() && line.back() == '\r') line.pop_back();          // (BufRead::lines strips "\r\n" as well)
        at = nl + 1;
        const size_t head = line.find('\t'), tail = line.rfind('\t');
        if (head == std::string::npos) return {GBWT_HIP_INVALID_DATA, "Name line missing last field"};   // (one field: next_back finds nothing)
        uint64_t id = 0, len = 0;
        if (!parse_names_number(line.substr(0, head), id) || !parse_names_number(line.substr(tail + 1), len))
            return {GBWT_HIP_INVALID_DATA, "invalid digit found in string: " + line};
        ids.push_back(id); lens.push_back(len);
    }
    if (ids.empty()) return {GBWT_HIP_INVALID_DATA, "No path names found"};
    return {};
}

inline FileCheck read_whole_file(const std::string &path, std::string &text) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return {GBWT_HIP_IO_ERROR, "cannot open " + path};
    char buffer[1 << 16];
    size_t got;
    while ((got = std::fread(buffer, 1, sizeof(buffer), f)) != 0) text.append(buffer, got);
    const bool broken = std::ferror(f) != 0;
    std::fclose(f);
    if (broken) return {GBWT_HIP_IO_ERROR, "cannot read " + path};
    return {};
}

inline FileCheck read_names(const std::string &names_path, std::vector<uint64_t> &ids, std::vector<uint64_t> &lens) {
    std::string text;
    const FileCheck opened = read_whole_file(names_path, text);
    return opened.ok() ? parse_names(text, ids, lens) : opened;
}

inline std::string invalid_length(uint64_t path_id, uint64_t expected, const std::string &got) {
    return "Invalid length for path " + std::to_string(path_id) + ": expected " + std::to_string(expected) + ", got " + got;
}

// GBZ::path gives nothing for an id the index lacks: extract_path is the endmarker alone, and the length check of the reference fails
inline FileCheck check_paths_exist(uint64_t sequences, const std::vector<uint64_t> &ids, const std::vector<uint64_t> &lens) {
    for (size_t k = 0; k < ids.size(); k++)
        if (!path_exists(sequences, ids[k])) return {GBWT_HIP_INVALID_DATA, invalid_length(ids[k], lens[k], "0 (no such path)")};
    return {};
}

// The walked bases of every path against its line.  rows: the ids.size() + 1 row offsets of a text with one endmarker behind every row
inline FileCheck check_walked_lengths(const std::vector<uint64_t> &ids, const std::vector<uint64_t> &lens, const uint64_t *rows) {
    for (size_t k = 0; k < ids.size(); k++) {
        const uint64_t walked = rows[k + 1] - rows[k] - 1;
        if (walked != lens[k]) return {GBWT_HIP_INVALID_DATA, invalid_length(ids[k], lens[k], std::to_string(walked))};
    }
    return {};
}

}  // namespace gbwt_hip
