// capi_gfa_build.hip -- construction from GFA over the C ABI (include/gbwt_hip.h, "construction from GFA"): the parse of gfa_parse.hip,
// the metadata of gfa_meta.hpp, the records of build.hip over the rows the parse left in HBM, and the open behind them.
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "build.hpp"
#include "capi_internal.hpp"
#include "gfa_meta.hpp"
#include "gfa_parse.hpp"
#include "hip_raii.hpp"

using namespace gbwt_hip;

namespace {

gbwt_hip_status check_call(const void *input, const char *what, uint32_t flags, gbwt_hip_index **out) {
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = nullptr;
    if (!input) return fail(GBWT_HIP_BAD_ARGUMENT, std::string("null ") + what);
    return check_open_flags(flags);
}

gbwt_hip_status refuse(uint64_t line, uint32_t code) {
    const std::string at = "GFA line " + std::to_string(line) + ": ";
    switch (code) {
        case GFA_ERR_CR: return fail(GBWT_HIP_INVALID_DATA, at + "a carriage return");
        case GFA_ERR_MALFORMED: return fail(GBWT_HIP_INVALID_DATA, at + "too few fields for its kind (S: 3, L: 5, P: 3, W: 7)");
        case GFA_ERR_NAME: return fail(GBWT_HIP_UNSUPPORTED, at + "the segment name is not a node id (a decimal number in 1 .. 2^31 - 1 without a leading zero); other names need a "
                                                                   "node-to-segment translation, which is not supported");
        case GFA_ERR_SEQUENCE: return fail(GBWT_HIP_INVALID_DATA, at + "a segment without a sequence");
        case GFA_ERR_STEP: return fail(GBWT_HIP_INVALID_DATA, at + "a step that is not a node id (1 .. 2^31 - 1, no leading zero) with its orientation");
        case GFA_ERR_UNKNOWN_SEGMENT: return fail(GBWT_HIP_INVALID_DATA, at + "a step names a segment without an S-line");
        case GFA_ERR_DUPLICATE: return fail(GBWT_HIP_INVALID_DATA, at + "the second S-line of its segment");
        case GFA_ERR_EMPTY_NAME: return fail(GBWT_HIP_INVALID_DATA, at + "a segment with an empty name");
        case GFA_ERR_LONG_NAME: return fail(GBWT_HIP_UNSUPPORTED, at + "a segment name of more than 255 bytes is not supported");
        case GFA_ERR_NAMED_STEP: return fail(GBWT_HIP_INVALID_DATA, at + "a step that is not a segment name with its orientation");
        case GFA_ERR_DUPLICATE_NAME: return fail(GBWT_HIP_INVALID_DATA, at + "a later S-line of its segment name");
        default: return fail(GBWT_HIP_INVALID_DATA, at + "refused");
    }
}

// NULL: the call without options
gbwt_hip_status check_options(const gbwt_hip_gfa_options *opts, GfaParseOptions &parsed) {
    parsed = GfaParseOptions();
    if (!opts) return GBWT_HIP_OK;
    if (opts->reserved[0] != 0 || opts->reserved[1] != 0) return fail(GBWT_HIP_BAD_ARGUMENT, "options: reserved must be 0");
    if (opts->translate > GBWT_HIP_GFA_TRANSLATE_ALWAYS) return fail(GBWT_HIP_BAD_ARGUMENT, "options: translate is one of GBWT_HIP_GFA_TRANSLATE_NEVER | _AUTO | _ALWAYS");
    if (opts->translate == GBWT_HIP_GFA_TRANSLATE_NEVER && opts->max_node_length != 0)
        return fail(GBWT_HIP_BAD_ARGUMENT, "options: max_node_length > 0 chops segments, which needs a translation (GBWT_HIP_GFA_TRANSLATE_AUTO or _ALWAYS)");
    parsed.max_node_length = opts->max_node_length; parsed.translate = opts->translate;
    return GBWT_HIP_OK;
}

gbwt_hip_status build_from_text(const char *text, uint64_t len, double read_ms, const GfaParseOptions &options, int device, uint32_t flags, gbwt_hip_index **out) {
    gbwt_hip_status st = require_device();
    if (st != GBWT_HIP_OK) return st;
    try {
        HIP_CHECK(hipSetDevice(device));
        Stream stream;
        GfaDeviceParse parse(text, len, stream.s, options);
        parse.rows();

        // metadata, from the few bytes of the name fields; its refusals and the device's are one list in file order
        const auto t_meta = Clock::now();
        HostIndex meta;
        std::vector<GfaPathFields> fields;
        fields.reserve(parse.path_lines.size());
        for (const GfaPathLine &p : parse.path_lines) fields.push_back(gfa_path_fields(text, p));
        const uint64_t stop = parse.refusal ? parse.refusal.line - 1 : ~uint64_t(0);
        const GfaMetaRefusal bad = assemble_gfa_metadata(fields, stop, meta);
        std::string reference_samples;
        bool have_reference_samples = false;
        for (const auto &h : parse.header_lines)
            if (!have_reference_samples) have_reference_samples = gfa_reference_samples(std::string_view(text + h.first, h.second - h.first), reference_samples);
        const double metadata_ms = ms_since(t_meta);
        if (bad && (!parse.refusal || bad.line < parse.refusal.line)) return fail(GBWT_HIP_INVALID_DATA, "GFA line " + std::to_string(bad.line) + ": " + bad.what);
        if (parse.refusal) return refuse(parse.refusal.line, parse.refusal.code);

        const uint64_t n_paths = parse.n_paths, steps = parse.row_nodes;      // (translated: the nodes of the steps)
        st = check_build_sizes(n_paths, steps, 1);
        if (st != GBWT_HIP_OK) return st;
        const uint64_t min_node = parse.min_node & ~uint64_t(1), max_node = parse.max_node | uint64_t(1);
        if (steps) {
            st = check_build_range(min_node, max_node);
            if (st != GBWT_HIP_OK) return st;
        }
        Strings labels;
        uint64_t graph_nodes = 0;
        parse.labels(labels, graph_nodes);
        GfaTranslation translation;
        parse.translation(translation);
        parse.release_all_but_rows();             // the ranking holds 40 B per slot: the text and the tables of the parse are gone before it starts

        BuildOutput o;
        if (steps == 0) build_without_visits(2 * n_paths, o);
        else build_records_on_device(BuildInput{parse.d_offsets(), parse.d_nodes(), n_paths, steps, true, min_node, max_node}, o, stream.s);

        const auto t_open = Clock::now();
        std::unique_ptr<gbwt_hip_index> ix = handle_from_build(o, true, device, flags);
        HostIndex &h = ix->host;
        if (have_reference_samples) { meta.tags.emplace_back("reference_samples", reference_samples); meta.gbz_tags.emplace_back("reference_samples", reference_samples); }
        adopt_metadata(h, std::move(meta));                                  // (assemble_gfa_metadata always says has_metadata; the graph comes from the parse)
        const bool translated = parse.translated && steps != 0;             // (without visits there are no nodes to map)
        if (translated) fill_gfa_translated_graph(h, std::move(labels), graph_nodes, std::move(translation.names), std::move(translation.starts), translation.mapping_len);
        else fill_gfa_graph(h, std::move(labels), graph_nodes);

        gbwt_hip_build_info b = build_info_of(o);
        gbwt_hip_gfa_info g{};
        const GfaCounts &c = parse.counts;
        g.bytes = c.bytes; g.lines = c.lines; g.headers = c.headers; g.segments = c.segments; g.links = c.links; g.p_lines = c.p_lines; g.w_lines = c.w_lines;
        g.ignored_lines = c.ignored_lines; g.steps = c.steps; g.label_bytes = c.label_bytes; g.tile_bytes = GFA_TILE_BYTES; g.peak_parse_bytes = parse.peak_bytes;
        g.structure_ms = parse.structure_ms; g.steps_ms = parse.steps_ms; g.labels_ms = parse.labels_ms;
        g.read_ms = read_ms; g.upload_ms = parse.upload_ms; g.metadata_ms = metadata_ms;

        gbwt_hip_gfa_translation_info tr{};
        tr.segments = c.segments;
        if (translated) {
            tr.translated = 1; tr.nodes = parse.total_nodes; tr.chopped_segments = parse.chopped_segments; tr.unvisited_segments = parse.unvisited_segments;
            tr.name_bytes = parse.name_bytes; tr.table_bytes = parse.table_bytes; tr.names_ms = parse.names_ms; tr.expand_ms = parse.expand_ms;
        }

        st = open_host_index(std::move(ix), out, t_open);
        if (st != GBWT_HIP_OK) return st;
        b.open_ms = ms_since(t_open);
        (*out)->build_info = b;
        (*out)->gfa_info = g;
        (*out)->gfa_translation_info = tr;
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e, "the construction");
    }
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_build_from_gfa_text(const char *text, uint64_t len, int device, uint32_t flags, gbwt_hip_index **out) {
    return gbwt_hip_build_from_gfa_text_opts(text, len, nullptr, device, flags, out);       // (no options: the defaults)
}

gbwt_hip_status gbwt_hip_build_from_gfa_text_opts(const char *text, uint64_t len, const gbwt_hip_gfa_options *opts, int device, uint32_t flags, gbwt_hip_index **out) {
    GBWT_HIP_GUARD_BEGIN
    gbwt_hip_status st = check_call(len ? static_cast<const void *>(text) : static_cast<const void *>(""), "text", flags, out);
    if (st != GBWT_HIP_OK) return st;
    GfaParseOptions options;
    st = check_options(opts, options);
    if (st != GBWT_HIP_OK) return st;
    return build_from_text(text, len, 0.0, options, device, flags, out);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_build_from_gfa_opts(const char *path, const gbwt_hip_gfa_options *opts, int device, uint32_t flags, gbwt_hip_index **out) {
    GBWT_HIP_GUARD_BEGIN
    gbwt_hip_status st = check_call(path, "path", flags, out);
    if (st != GBWT_HIP_OK) return st;
    GfaParseOptions options;
    st = check_options(opts, options);
    if (st != GBWT_HIP_OK) return st;
    const auto t0 = Clock::now();
    const GfaFile file(path);                     // (IoError: before the device is touched)
    return build_from_text(file.data(), file.size(), ms_since(t0), options, device, flags, out);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_gfa_translation_info(const gbwt_hip_index *ix, gbwt_hip_gfa_translation_info *out) {
    GBWT_HIP_GUARD_BEGIN
    return last_info(ix, out, &gbwt_hip_index::gfa_translation_info);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_build_from_gfa(const char *path, int device, uint32_t flags, gbwt_hip_index **out) {
    return gbwt_hip_build_from_gfa_opts(path, nullptr, device, flags, out);
}

gbwt_hip_status gbwt_hip_last_gfa_info(const gbwt_hip_index *ix, gbwt_hip_gfa_info *out) {
    GBWT_HIP_GUARD_BEGIN
    return last_info(ix, out, &gbwt_hip_index::gfa_info);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_parse_gfa(const char *path, gbwt_hip_gfa_info *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!path || !out) return fail(GBWT_HIP_BAD_ARGUMENT, "null argument");
    const auto t0 = Clock::now();
    const GfaFile file(path);
    const GfaCounts c = count_gfa_on_host(file.data(), file.size());
    gbwt_hip_gfa_info g{};
    g.bytes = c.bytes; g.lines = c.lines; g.headers = c.headers; g.segments = c.segments; g.links = c.links; g.p_lines = c.p_lines; g.w_lines = c.w_lines;
    g.ignored_lines = c.ignored_lines; g.steps = c.steps; g.label_bytes = c.label_bytes; g.tile_bytes = GFA_TILE_BYTES;
    g.read_ms = ms_since(t0);
    *out = g;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

}  // extern "C"
