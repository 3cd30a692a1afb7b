// gfa_parse.hpp -- GFA text to rows of nodes and node labels on the device (gfa_parse.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "gfa_meta.hpp"
#include "host_index.hpp"

namespace gbwt_hip {

// One wave reads one tile: 64 lanes x 16 bytes.  Every pass over the text is cut into these.
constexpr uint32_t GFA_TILE_BYTES = 1024;
// Zero bytes behind the text in HBM (on top of the rest of its last tile): a token is read past its marker without a bounds test
constexpr uint32_t GFA_TEXT_PAD = 16;
// hipcub counts in int
constexpr uint64_t GFA_MAX_LINES = 0x7FFFFFFFull;

// What a refusal was about.  The error word of the device is (line << 8 | code), lowered with atomicMin: the FIRST offending line in file
// order wins, and on one line the smallest code.
enum GfaErrorCode : uint32_t {
    GFA_ERR_CR = 1,              // a carriage return
    GFA_ERR_MALFORMED = 2,       // a line of a known kind without its fields
    GFA_ERR_NAME = 3,            // an S name that is not a node id (GBWT_HIP_UNSUPPORTED)
    GFA_ERR_SEQUENCE = 4,        // an S line without a sequence
    GFA_ERR_STEP = 5,            // a step that is not a node id with its orientation
    GFA_ERR_UNKNOWN_SEGMENT = 6, // a step without an S line
    GFA_ERR_DUPLICATE = 7,       // the second S line of an id
    // a translated parse only
    GFA_ERR_EMPTY_NAME = 8,      // an S line with an empty name
    GFA_ERR_LONG_NAME = 9,       // an S name of more than GFA_MAX_NAME bytes (GBWT_HIP_UNSUPPORTED)
    GFA_ERR_NAMED_STEP = 10,     // a step that is not a name with its orientation
    GFA_ERR_DUPLICATE_NAME = 11, // a later S line of a name
    GFA_ERR_NONE = 0xFF
};

struct GfaRefusal {
    uint64_t line = 0;           // 1-based; 0: none
    uint32_t code = GFA_ERR_NONE;
    explicit operator bool() const { return line != 0; }
};

// How the segments become nodes (include/gbwt_hip.h, gbwt_hip_gfa_options)
struct GfaParseOptions {
    uint32_t max_node_length = 0;             // 0: nothing is chopped
    uint32_t translate = 0;                   // GBWT_HIP_GFA_TRANSLATE_*
};

// What a translated parse leaves for the HostIndex: the names of the visited segments (empty for the others) and the first node of each
struct GfaTranslation {
    Strings names;
    Words starts;
    uint64_t mapping_len = 0;
};

// The parse of one text on the current device.  rows(): structure and steps; labels(): the node labels, once the rows stand;
// release_all_but_rows(): what the construction must not find in its way.  Throws HipError / Unsupported.
class GfaDeviceParse {
public:
    GfaDeviceParse(const char *text, uint64_t len, hipStream_t s, GfaParseOptions options = GfaParseOptions());
    ~GfaDeviceParse();
    GfaDeviceParse(const GfaDeviceParse &) = delete;
    GfaDeviceParse &operator=(const GfaDeviceParse &) = delete;

    void rows();
    void labels(Strings &out, uint64_t &graph_nodes);
    void translation(GfaTranslation &out);    // of a translated parse, behind labels()
    void release_all_but_rows();

    GfaCounts counts;
    GfaRefusal refusal;                       // the first offending line the device found (rows())
    uint64_t n_paths = 0;
    std::vector<GfaPathLine> path_lines;      // in path order: the P-lines, then the W-lines
    std::vector<std::pair<uint64_t, uint64_t>> header_lines;   // [start, end) of every H-line
    const uint64_t *d_offsets() const;        // u64[n_paths + 1]
    const uint32_t *d_nodes() const;          // u32[row_nodes]
    uint32_t min_node = 0, max_node = 0;      // over the steps (only with steps)
    uint64_t peak_bytes = 0;
    double upload_ms = 0;
    float structure_ms = 0, steps_ms = 0, labels_ms = 0;
    // A translated parse (rows() decides: ALWAYS, or AUTO over a text that needs it; never for a text without S-lines): segments are the
    // S-lines in file order, `row_nodes` the length of d_nodes() -- every step expanded to the nodes of its segment --, counts.steps the steps
    bool translated = false;
    uint64_t row_nodes = 0, total_nodes = 0, chopped_segments = 0, unvisited_segments = 0, name_bytes = 0, table_bytes = 0;
    float names_ms = 0, expand_ms = 0;

private:
    struct Impl;
    Impl *impl;
};

}  // namespace gbwt_hip
