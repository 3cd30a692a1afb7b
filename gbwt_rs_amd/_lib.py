"""Loader + ctypes signatures of libgbwt_hip.so (the C ABI declared in include/gbwt_hip.h).

The shared library is built in-tree by `make -C gbwt_rs_amd/csrc` (see __graft_entry__.build).
There is no Python or CPU fallback: if the library is missing, importing this module's `lib()`
raises, and on a box without a HIP device every compute call returns GBWT_HIP_NO_DEVICE.
"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.environ.get("GBWT_HIP_LIB") or os.path.join(CSRC, "libgbwt_hip.so")   # GBWT_HIP_LIB: A/B runs of two builds (tools/)
HEADER = os.path.join(os.path.dirname(HERE), "include", "gbwt_hip.h")

OPEN_EXTRACT, OPEN_SEARCH, OPEN_GFA, OPEN_ALL = 1, 2, 4, 7     # gbwt_hip_open_*_flags
OK, INVALID_DATA, IO_ERROR, BAD_ARGUMENT, NO_DEVICE, DEVICE_ERROR, CAPACITY, UNSUPPORTED = range(8)
STATUS_NAMES = ["OK", "INVALID_DATA", "IO_ERROR", "BAD_ARGUMENT", "NO_DEVICE", "DEVICE_ERROR", "CAPACITY", "UNSUPPORTED"]


class Pos(C.Structure):
    _fields_ = [("node", C.c_uint64), ("offset", C.c_uint64)]


class State(C.Structure):
    _fields_ = [("node", C.c_uint64), ("start", C.c_uint64), ("end", C.c_uint64)]


class BdState(C.Structure):
    _fields_ = [("forward", State), ("reverse", State)]


class Stats(C.Structure):
    _fields_ = [("size", C.c_uint64), ("sequences", C.c_uint64), ("alphabet_size", C.c_uint64),
                ("alphabet_offset", C.c_uint64), ("records", C.c_uint64), ("data_bytes", C.c_uint64),
                ("paths", C.c_uint64), ("bidirectional", C.c_uint32), ("has_metadata", C.c_uint32),
                ("is_gbz", C.c_uint32), ("has_translation", C.c_uint32), ("max_record_len", C.c_uint64),
                ("max_outdegree", C.c_uint64)]


class OpenTimes(C.Structure):
    _fields_ = [("parse_ms", C.c_double), ("upload_ms", C.c_double), ("sample_ms", C.c_double), ("total_ms", C.c_double),
                ("samples", C.c_uint64), ("checkpoint_walkers", C.c_uint64), ("checkpoint_orphans", C.c_uint64), ("checkpoint_sampling", C.c_uint32),
                ("checkpoint_rounds", C.c_uint32), ("line_sizes_ms", C.c_double)]


class Memory(C.Structure):
    _fields_ = [("index_device_bytes", C.c_uint64), ("index_host_bytes", C.c_uint64), ("workspace_device_bytes", C.c_uint64),
                ("rows_bytes", C.c_uint64), ("text_bytes", C.c_uint64), ("rows_chunks", C.c_uint64)]


class UniqueId(C.Structure):
    _fields_ = [("bytes", C.c_ubyte * 128)]       # binary: NOT c_char (a c_char array reads as a C string and stops at the first NUL)


class CommStats(C.Structure):
    _fields_ = [("ms", C.c_double), ("bytes", C.c_uint64), ("staged_send", C.c_uint32), ("reserved", C.c_uint32)]


class Paths(C.Structure):
    _fields_ = [("d_offsets", C.c_void_p), ("d_nodes", C.c_void_p), ("total", C.c_uint64), ("n", C.c_uint64)]


class States(C.Structure):
    _fields_ = [("d_states", C.c_void_p), ("d_valid", C.c_void_p), ("n", C.c_uint64)]


class Lines(C.Structure):
    _fields_ = [("d_text", C.c_void_p), ("d_line_offsets", C.c_void_p), ("total", C.c_uint64), ("n", C.c_uint64)]


class Components(C.Structure):
    _fields_ = [("d_component", C.c_void_p), ("d_offsets", C.c_void_p), ("d_nodes", C.c_void_p), ("d_path_component", C.c_void_p),
                ("min_node", C.c_uint64), ("slots", C.c_uint64), ("components", C.c_uint64), ("nodes", C.c_uint64), ("paths", C.c_uint64)]


class ComponentsTimes(C.Structure):
    _fields_ = [("hook_ms", C.c_float), ("jump_ms", C.c_float), ("shape_ms", C.c_float), ("hook_launches", C.c_uint32),
                ("jump_launches", C.c_uint32), ("shape_launches", C.c_uint32)]


class EdgeRows(C.Structure):
    _fields_ = [("d_offsets", C.c_void_p), ("d_edges", C.c_void_p), ("d_valid", C.c_void_p), ("total", C.c_uint64), ("n", C.c_uint64)]


class GraphText(C.Structure):
    _fields_ = [("d_text", C.c_void_p), ("header_bytes", C.c_uint64), ("segment_bytes", C.c_uint64), ("link_bytes", C.c_uint64),
                ("segments", C.c_uint64), ("links", C.c_uint64)]


class SuffixArray(C.Structure):
    _fields_ = [("d_sa", C.c_void_p), ("d_bwt", C.c_void_p), ("total", C.c_uint64), ("bwt_runs", C.c_uint64)]


class SuffixArrayInfo(C.Structure):
    _fields_ = [("n", C.c_uint64), ("peak_scratch_bytes", C.c_uint64), ("planned_scratch_bytes", C.c_uint64), ("bwt_runs", C.c_uint64),
                ("active", C.c_uint64 * 64), ("rounds", C.c_uint32), ("rank_bits", C.c_uint32), ("text_ms", C.c_float), ("pack_ms", C.c_float),
                ("rank_ms", C.c_float), ("output_ms", C.c_float), ("round_ms", C.c_float * 64)]


FM_COUNT_ONLY = 1     # gbwt_hip_fm_build_* flags


class FmIndexInfo(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("n", "sigma", "block_rows", "blocks", "primary", "index_bytes", "planned_index_bytes", "sa_bytes", "peak_scratch_bytes",
                                                "planned_scratch_bytes", "queries", "last_patterns", "last_steps", "last_total")] + \
               [(name, C.c_uint32) for name in ("packed", "count_only", "path_level", "reserved")] + \
               [(name, C.c_float) for name in ("suffix_array_ms", "histogram_ms", "codes_ms", "counts_ms", "fill_ms", "narrow_ms", "last_count_ms", "last_fill_ms")]


class FmLocated(C.Structure):
    _fields_ = [("d_offsets", C.c_void_p), ("d_values", C.c_void_p), ("d_ranges", C.c_void_p), ("total", C.c_uint64), ("m", C.c_uint64)]


STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH = 1, 2, 3     # gbwt_hip_fm_seed_options.strands, gbwt_hip_fm_seed.strand


class FmSeedOptions(C.Structure):
    _fields_ = [("min_length", C.c_uint32), ("strands", C.c_uint32), ("max_occurrences", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class FmSeed(C.Structure):
    _fields_ = [("lo", C.c_uint64), ("hi", C.c_uint64), ("start", C.c_uint32), ("end", C.c_uint32), ("strand", C.c_uint32), ("reserved", C.c_uint32)]


class FmSeedInfo(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("requests", "reads", "read_bytes", "anchors", "refined_ends", "steps", "seeds", "hits", "over_max", "planned_scratch_bytes",
                                                "peak_scratch_bytes")] + \
               [(name, C.c_uint32) for name in ("stride", "strands")] + \
               [(name, C.c_float) for name in ("idle_share", "anchor_ms", "refine_ms", "emit_ms", "hits_ms", "reserved")]


class FmSeedRows(C.Structure):
    _fields_ = [("d_read_offsets", C.c_void_p), ("d_seeds", C.c_void_p), ("d_hit_offsets", C.c_void_p), ("d_hits", C.c_void_p), ("total_seeds", C.c_uint64), ("total_hits", C.c_uint64),
                ("m", C.c_uint64)]


class FmChainOptions(C.Structure):
    _fields_ = [("max_gap", C.c_uint32), ("max_skew", C.c_uint32), ("gap_cost", C.c_uint32), ("min_score", C.c_uint32), ("max_matches", C.c_uint64), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class FmChain(C.Structure):
    _fields_ = [("text_start", C.c_uint64), ("text_end", C.c_uint64)] + \
               [(name, C.c_uint32) for name in ("read_start", "read_end", "score", "matches", "strand", "path")]


class FmChainMatch(C.Structure):
    _fields_ = [("y", C.c_uint64), ("x", C.c_uint32), ("w", C.c_uint32)]


class FmChainInfo(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("requests", "items", "matches", "skipped_items", "pairs", "chains", "chain_matches", "tile_matches", "planned_scratch_bytes",
                                                "peak_scratch_bytes", "path_offset_bytes")] + \
               [(name, C.c_float) for name in ("seeds_ms", "expand_ms", "sort_ms", "dp_ms", "peel_ms", "fill_ms")]


class FmChainRows(C.Structure):
    _fields_ = [("d_read_offsets", C.c_void_p), ("d_chains", C.c_void_p), ("d_match_offsets", C.c_void_p), ("d_matches", C.c_void_p), ("total_chains", C.c_uint64),
                ("total_matches", C.c_uint64), ("m", C.c_uint64)]


ALIGN_OK, ALIGN_WIDE, ALIGN_NONE = 0, 1, 2     # gbwt_hip_fm_alignment.status


class FmAlignOptions(C.Structure):
    _fields_ = [("band", C.c_uint32), ("max_width", C.c_uint32), ("max_alignments", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class FmAlignment(C.Structure):
    _fields_ = [("text_start", C.c_uint64), ("text_end", C.c_uint64)] + \
               [(name, C.c_uint32) for name in ("chain", "edit_distance", "width", "status", "strand", "path")]


class FmAlignInfo(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("requests", "items", "chains", "alignments", "wide", "unreachable", "cells", "cigar_ops", "lds_alignments", "global_alignments",
                                                "tile_bytes", "text_bytes", "planned_scratch_bytes", "peak_scratch_bytes")] + \
               [(name, C.c_float) for name in ("chains_ms", "select_ms", "dp_ms", "trace_ms", "rows_ms", "reserved")]


class FmAlignmentRows(C.Structure):
    _fields_ = [("d_read_offsets", C.c_void_p), ("d_alignments", C.c_void_p), ("d_cigar_offsets", C.c_void_p), ("d_cigars", C.c_void_p), ("total_alignments", C.c_uint64),
                ("total_cigars", C.c_uint64), ("m", C.c_uint64)]


class ReferencePath(C.Structure):
    _fields_ = [("path_id", C.c_uint64), ("len", C.c_uint64), ("first", C.c_uint64), ("count", C.c_uint64)]


class ReferencePosition(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("pos", Pos)]


class Located(C.Structure):
    _fields_ = [("d_offsets", C.c_void_p), ("d_ids", C.c_void_p), ("d_valid", C.c_void_p), ("total", C.c_uint64), ("n", C.c_uint64)]


class LocateInfo(C.Structure):
    _fields_ = [("built", C.c_uint32), ("interval", C.c_uint32), ("sampled_records", C.c_uint64), ("table_positions", C.c_uint64),
                ("end_entries", C.c_uint64), ("device_bytes", C.c_uint64), ("build_ms", C.c_double), ("build_launches", C.c_uint32),
                ("reserved", C.c_uint32)]


class BuildInfo(C.Structure):
    _fields_ = [("visits", C.c_uint64), ("sequences", C.c_uint64), ("records", C.c_uint64), ("data_bytes", C.c_uint64), ("peak_scratch_bytes", C.c_uint64),
                ("rounds", C.c_uint32), ("built", C.c_uint32), ("expand_ms", C.c_float), ("rank_ms", C.c_float), ("edges_ms", C.c_float),
                ("encode_ms", C.c_float), ("open_ms", C.c_double)]


class GfaInfo(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("bytes", "lines", "headers", "segments", "links", "p_lines", "w_lines", "ignored_lines", "steps", "label_bytes",
                                                "tile_bytes", "peak_parse_bytes")] + \
               [("structure_ms", C.c_float), ("steps_ms", C.c_float), ("labels_ms", C.c_float), ("reserved", C.c_float),
                ("read_ms", C.c_double), ("upload_ms", C.c_double), ("metadata_ms", C.c_double)]


GFA_TRANSLATE_NEVER, GFA_TRANSLATE_AUTO, GFA_TRANSLATE_ALWAYS = 0, 1, 2     # gbwt_hip_gfa_options.translate


class GfaOptions(C.Structure):
    _fields_ = [("max_node_length", C.c_uint32), ("translate", C.c_uint32), ("reserved", C.c_uint64 * 2)]


class GfaTranslationInfo(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("translated", "segments", "nodes", "chopped_segments", "unvisited_segments", "name_bytes", "table_bytes")] + \
               [("names_ms", C.c_float), ("expand_ms", C.c_float), ("reserved", C.c_float * 2)]


MERGE_AUTO, MERGE_REBUILD, MERGE_INSERT = 0, 1, 2     # gbwt_hip_merge_options.algorithm


class MergeOptions(C.Structure):
    _fields_ = [("algorithm", C.c_uint32), ("reserved32", C.c_uint32), ("reserved", C.c_uint64 * 2)]


class MergeInfo(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("visits", "sequences", "records", "data_bytes", "peak_scratch_bytes", "walked_sequences", "walked_steps")] + \
               [(name, C.c_uint32) for name in ("algorithm_used", "walked_input", "merged", "rounds")] + \
               [(name, C.c_float) for name in ("walk_ms", "decode_ms", "interleave_ms", "edges_ms", "encode_ms")] + \
               [("metadata_ms", C.c_double), ("open_ms", C.c_double)]


REMOVE_AUTO, REMOVE_REBUILD, REMOVE_DELETE = 0, 1, 2   # gbwt_hip_remove_options.algorithm


class RemoveOptions(C.Structure):
    _fields_ = [("algorithm", C.c_uint32), ("reserved32", C.c_uint32), ("reserved", C.c_uint64 * 2)]


class RemoveInfo(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("visits", "sequences", "records", "data_bytes", "peak_scratch_bytes", "removed_sequences", "removed_steps")] + \
               [(name, C.c_uint32) for name in ("algorithm_used", "removed", "rounds", "reserved32")] + \
               [(name, C.c_float) for name in ("walk_ms", "decode_ms", "compact_ms", "edges_ms", "encode_ms")] + \
               [("metadata_ms", C.c_double), ("open_ms", C.c_double)]


_p, _u64, _int = C.c_void_p, C.c_uint64, C.c_int

SIGNATURES = {
    "gbwt_hip_last_error": (C.c_char_p, []),
    "gbwt_hip_device_count": (_int, []),
    "gbwt_hip_open_file": (_int, [C.c_char_p, _int, C.POINTER(_p)]),
    "gbwt_hip_parse_file": (_int, [C.c_char_p, C.POINTER(Stats)]),
    "gbwt_hip_open_records": (_int, [_p, _u64, _p, _u64, _u64, _u64, _u64, _u64, _int, _int, C.POINTER(_p)]),
    "gbwt_hip_open_file_flags": (_int, [C.c_char_p, _int, C.c_uint32, C.POINTER(_p)]),
    "gbwt_hip_open_records_flags": (_int, [_p, _u64, _p, _u64, _u64, _u64, _u64, _u64, _int, _int, C.c_uint32, C.POINTER(_p)]),
    "gbwt_hip_close": (None, [_p]),
    "gbwt_hip_get_stats": (_int, [_p, C.POINTER(Stats)]),
    "gbwt_hip_get_open_times": (_int, [_p, C.POINTER(OpenTimes)]),
    "gbwt_hip_memory_usage": (_int, [_p, _p, C.POINTER(Memory)]),
    "gbwt_hip_last_lines_ms": (_int, [_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "gbwt_hip_workspace_create": (_int, [_p, C.POINTER(_p)]),
    "gbwt_hip_workspace_destroy": (None, [_p]),
    "gbwt_hip_workspace_stream": (_p, [_p]),
    "gbwt_hip_workspace_tune": (_int, [_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "gbwt_hip_extract": (_int, [_p, _p, _p, _u64, _p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_extract_device": (_int, [_p, _p, _p, _u64, C.POINTER(Paths)]),
    "gbwt_hip_extract_part_device": (_int, [_p, _p, _p, _u64, C.c_uint32, C.c_uint32, C.POINTER(Paths)]),
    "gbwt_hip_copy_result": (_int, [_p, _p, _p, _p, _u64]),
    "gbwt_hip_extract_paths": (_int, [_p, _p, _p, _u64, _int, _p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_start": (_int, [_p, _p, _p, _u64, _p, _p]),
    "gbwt_hip_forward": (_int, [_p, _p, _p, _u64, _p, _p]),
    "gbwt_hip_backward": (_int, [_p, _p, _p, _u64, _p, _p]),
    "gbwt_hip_find": (_int, [_p, _p, _p, _u64, _p, _p]),
    "gbwt_hip_extend": (_int, [_p, _p, _p, _p, _u64, _p, _p]),
    "gbwt_hip_bd_find": (_int, [_p, _p, _p, _u64, _p, _p]),
    "gbwt_hip_extend_forward": (_int, [_p, _p, _p, _p, _u64, _p, _p]),
    "gbwt_hip_follow": (_int, [_p, _p, _p, _u64, _int, _p, _p, _u64, _p, _p]),
    "gbwt_hip_extend_backward": (_int, [_p, _p, _p, _p, _u64, _p, _p]),
    "gbwt_hip_search": (_int, [_p, _p, _p, _u64, _u64, _p, _p]),
    "gbwt_hip_bd_search": (_int, [_p, _p, _p, _u64, _u64, _u64, _p, _p]),
    "gbwt_hip_search_device": (_int, [_p, _p, _p, _u64, _u64, C.POINTER(States)]),
    "gbwt_hip_bd_search_device": (_int, [_p, _p, _p, _u64, _u64, _u64, C.POINTER(States)]),
    "gbwt_hip_path_lines": (_int, [_p, _p, _p, _u64, _int, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_path_lines_device": (_int, [_p, _p, _p, _u64, _int, C.POINTER(Lines)]),
    "gbwt_hip_segment_paths": (_int, [_p, _p, _p, _u64, _p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_write_gfa": (_int, [_p, _p, C.c_char_p]),
    "gbwt_hip_write_gfa_mode": (_int, [_p, _p, C.c_char_p, _int]),
    "gbwt_hip_path_sequences_device": (_int, [_p, _p, _p, _u64, _int, _int, C.POINTER(Lines)]),
    "gbwt_hip_path_sequences": (_int, [_p, _p, _p, _u64, _int, _int, _p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_node_sequence": (_int, [_p, _u64, _p, _u64, C.POINTER(_u64), C.POINTER(C.c_uint8)]),
    "gbwt_hip_write_sequences": (_int, [_p, _p, C.c_char_p, _p, _u64, _int]),
    "gbwt_hip_last_sequences_ms": (_int, [_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "gbwt_hip_tags_device": (_int, [_p, _p, _p, _u64, _p, _u64, _p, C.POINTER(_u64)]),
    "gbwt_hip_tags": (_int, [_p, _p, _p, _u64, _p, _u64, _p, C.POINTER(_u64), C.POINTER(_u64)]),
    "gbwt_hip_write_tag_array": (_int, [_p, _p, C.c_char_p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_last_tags_ms": (_int, [_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "gbwt_hip_suffix_array_text": (_int, [_int, _p, _u64, _int, _p, _p, C.POINTER(_u64)]),
    "gbwt_hip_suffix_array_text_device": (_int, [_int, _p, _u64, _int, _p, _p, _p, C.POINTER(_u64)]),
    "gbwt_hip_path_suffix_array_device": (_int, [_p, _p, _p, _u64, _int, C.POINTER(SuffixArray)]),
    "gbwt_hip_path_suffix_array": (_int, [_p, _p, _p, _u64, _int, _p, _p, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "gbwt_hip_write_suffix_array": (_int, [_p, _p, C.c_char_p, C.POINTER(_u64)]),
    "gbwt_hip_last_suffix_array_info": (_int, [_p, C.POINTER(SuffixArrayInfo)]),
    "gbwt_hip_fm_build_text": (_int, [_int, _p, _u64, _int, C.c_uint32, C.POINTER(_p)]),
    "gbwt_hip_fm_build_text_device": (_int, [_int, _p, _u64, _int, _p, C.c_uint32, _p, C.POINTER(_p)]),
    "gbwt_hip_path_fm_index": (_int, [_p, _p, _p, _u64, _int, C.c_uint32, C.POINTER(_p)]),
    "gbwt_hip_fm_close": (None, [_p]),
    "gbwt_hip_fm_info": (_int, [_p, C.POINTER(FmIndexInfo)]),
    "gbwt_hip_fm_count": (_int, [_p, _p, _p, _u64, _p]),
    "gbwt_hip_fm_locate": (_int, [_p, _p, _p, _u64, _p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_fm_graph_positions": (_int, [_p, _p, _p, _p, _p, _u64, _int, _p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_fm_count_device": (_int, [_p, _p, _p, _u64, _u64, C.POINTER(FmLocated)]),
    "gbwt_hip_fm_locate_device": (_int, [_p, _p, _p, _u64, _u64, C.POINTER(FmLocated)]),
    "gbwt_hip_fm_graph_positions_device": (_int, [_p, _p, _p, _p, _p, _u64, _u64, _int, C.POINTER(FmLocated)]),
    "gbwt_hip_fm_last_seed_info": (_int, [_p, C.POINTER(FmSeedInfo)]),
    "gbwt_hip_fm_seeds": (_int, [_p, _p, _p, _u64, C.POINTER(FmSeedOptions), _p, _p, _u64, C.POINTER(_u64), _p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_fm_seed_graph_positions": (_int, [_p, _p, _p, _p, _p, _u64, C.POINTER(FmSeedOptions), _p, _p, _u64, C.POINTER(_u64), _p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_fm_seeds_device": (_int, [_p, _p, _p, _u64, _u64, C.POINTER(FmSeedOptions), C.POINTER(FmSeedRows)]),
    "gbwt_hip_fm_seed_graph_positions_device": (_int, [_p, _p, _p, _p, _p, _u64, _u64, C.POINTER(FmSeedOptions), C.POINTER(FmSeedRows)]),
    "gbwt_hip_fm_last_chain_info": (_int, [_p, C.POINTER(FmChainInfo)]),
    "gbwt_hip_fm_chains": (_int, [_p, _p, _p, _u64, C.POINTER(FmSeedOptions), C.POINTER(FmChainOptions), _p, _p, _u64, C.POINTER(_u64), _p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_fm_chains_device": (_int, [_p, _p, _p, _u64, _u64, C.POINTER(FmSeedOptions), C.POINTER(FmChainOptions), C.POINTER(FmChainRows)]),
    "gbwt_hip_fm_set_text": (_int, [_p, _p, _u64]),
    "gbwt_hip_fm_set_text_device": (_int, [_p, _p, _u64, _p]),
    "gbwt_hip_fm_keep_path_text": (_int, [_p, _p, _p]),
    "gbwt_hip_fm_last_align_info": (_int, [_p, C.POINTER(FmAlignInfo)]),
    "gbwt_hip_fm_alignments": (_int, [_p, _p, _p, _u64, C.POINTER(FmSeedOptions), C.POINTER(FmChainOptions), C.POINTER(FmAlignOptions), _p, _p, _u64, C.POINTER(_u64), _p, _p, _u64,
                                      C.POINTER(_u64)]),
    "gbwt_hip_fm_alignments_device": (_int, [_p, _p, _p, _u64, _u64, C.POINTER(FmSeedOptions), C.POINTER(FmChainOptions), C.POINTER(FmAlignOptions), C.POINTER(FmAlignmentRows)]),
    "gbwt_hip_components_device": (_int, [_p, C.POINTER(Components)]),
    "gbwt_hip_weakly_connected_components": (_int, [_p, _p, _u64, _p, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "gbwt_hip_path_components": (_int, [_p, _p, _u64, _p]),
    "gbwt_hip_last_components_ms": (_int, [_p, C.POINTER(ComponentsTimes)]),
    "gbwt_hip_select_paths": (_int, [_p, _p, C.c_char_p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_write_sequences_contig": (_int, [_p, _p, C.c_char_p, C.c_char_p, _int]),
    "gbwt_hip_node_ids": (_int, [_p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_edges": (_int, [_p, _p, _p, _p, _u64, _int, _p, _p, _u64, C.POINTER(_u64), _p]),
    "gbwt_hip_edges_device": (_int, [_p, _p, _p, _p, _u64, _int, C.POINTER(EdgeRows)]),
    "gbwt_hip_segments": (_int, [_p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_node_segments": (_int, [_p, _p, _u64, _p, _p]),
    "gbwt_hip_links": (_int, [_p, _p, _p, _p, _u64, _int, _p, _p, _u64, C.POINTER(_u64), _p]),
    "gbwt_hip_links_device": (_int, [_p, _p, _p, _p, _u64, _int, C.POINTER(EdgeRows)]),
    "gbwt_hip_graph_lines_device": (_int, [_p, _p, C.POINTER(GraphText)]),
    "gbwt_hip_graph_lines": (_int, [_p, _p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_last_graph_ms": (_int, [_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "gbwt_hip_reference_sample_names": (_int, [_p, _int, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_reference_paths": (_int, [_p, _int, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_path_positions_device": (_int, [_p, _p, _p, _u64, _u64, C.POINTER(_p), C.POINTER(_p), C.POINTER(_u64)]),
    "gbwt_hip_path_positions": (_int, [_p, _p, _p, _u64, _u64, _p, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_reference_positions": (_int, [_p, _p, _u64, _p, _u64, C.POINTER(_u64), _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_last_positions_ms": (_int, [_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "gbwt_hip_last_positions_rounds": (_int, [_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "gbwt_hip_locate": (_int, [_p, _p, _p, _u64, _int, _p, _p, _u64, C.POINTER(_u64), _p]),
    "gbwt_hip_locate_device": (_int, [_p, _p, _p, _u64, _int, C.POINTER(Located)]),
    "gbwt_hip_locate_states_device": (_int, [_p, _p, _p, _p, _u64, _int, C.POINTER(Located)]),
    "gbwt_hip_locate_positions": (_int, [_p, _p, _p, _u64, _p, _p]),
    "gbwt_hip_last_locate_ms": (_int, [_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "gbwt_hip_locate_count_steps": (_int, [_p, _p, _p, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "gbwt_hip_locate_index_info": (_int, [_p, C.POINTER(LocateInfo)]),
    "gbwt_hip_build_from_paths": (_int, [_p, _p, _u64, _int, _int, C.c_uint32, C.POINTER(_p)]),
    "gbwt_hip_build_from_rows_device": (_int, [_p, _p, _u64, _int, _int, C.c_uint32, C.POINTER(_p)]),
    "gbwt_hip_records": (_int, [_p, _p, _u64, C.POINTER(_u64), _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_save": (_int, [_p, C.c_char_p]),
    "gbwt_hip_last_build_info": (_int, [_p, C.POINTER(BuildInfo)]),
    "gbwt_hip_build_from_gfa": (_int, [C.c_char_p, _int, C.c_uint32, C.POINTER(_p)]),
    "gbwt_hip_build_from_gfa_text": (_int, [_p, _u64, _int, C.c_uint32, C.POINTER(_p)]),
    "gbwt_hip_last_gfa_info": (_int, [_p, C.POINTER(GfaInfo)]),
    "gbwt_hip_build_from_gfa_opts": (_int, [C.c_char_p, C.POINTER(GfaOptions), _int, C.c_uint32, C.POINTER(_p)]),
    "gbwt_hip_build_from_gfa_text_opts": (_int, [_p, _u64, C.POINTER(GfaOptions), _int, C.c_uint32, C.POINTER(_p)]),
    "gbwt_hip_last_gfa_translation_info": (_int, [_p, C.POINTER(GfaTranslationInfo)]),
    "gbwt_hip_parse_gfa": (_int, [C.c_char_p, C.POINTER(GfaInfo)]),
    "gbwt_hip_merge": (_int, [_p, _p, C.POINTER(MergeOptions), C.c_uint32, C.POINTER(_p)]),
    "gbwt_hip_last_merge_info": (_int, [_p, C.POINTER(MergeInfo)]),
    "gbwt_hip_remove_paths": (_int, [_p, _p, _u64, C.POINTER(RemoveOptions), C.c_uint32, C.POINTER(_p)]),
    "gbwt_hip_last_remove_info": (_int, [_p, C.POINTER(RemoveInfo)]),
    "gbwt_hip_path_sums": (_int, [_p, _p, _p, _u64]),
    "gbwt_hip_path_hashes": (_int, [_p, _p, _p, _u64]),
    "gbwt_hip_copy_path": (_int, [_p, _p, _u64, _p, _u64, C.POINTER(_u64)]),
    "gbwt_hip_last_kernel_ms": (_int, [_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "gbwt_hip_last_query_ms": (_int, [_p, C.POINTER(C.c_float)]),
    "gbwt_hip_device_memory": (_int, [_int, C.POINTER(_u64), C.POINTER(_u64)]),
    "gbwt_hip_comm_unique_id": (_int, [C.POINTER(UniqueId)]),
    "gbwt_hip_comm_create": (_int, [C.POINTER(UniqueId), _int, _int, _int, C.POINTER(_p)]),
    "gbwt_hip_comm_destroy": (None, [_p]),
    "gbwt_hip_gather_rows": (_int, [_p, _p, _p, _int, _int, C.POINTER(Paths)]),
    "gbwt_hip_gather_lines": (_int, [_p, _p, _p, _int, _int, C.POINTER(Lines)]),
    "gbwt_hip_comm_last": (_int, [_p, C.POINTER(CommStats)]),
}

_lib = None


def lib():
    """The loaded C-ABI library.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `make -C {CSRC}` (or __graft_entry__.build()); "
                              "gbwt_rs_amd has no CPU fallback")
        # A process that uses torch AND this library must load torch FIRST: torch brings its own copy of the HIP runtime, and when
        # libgbwt_hip.so (linked against /opt/rocm's) has started the device before torch is imported, torch's runtime finds "No HIP
        # GPUs" (measured on the GPU box, round 5: a late `import torch` + .cuda() after the first extraction).  The other order works:
        # this library then binds to the runtime that is already in the process.  So the Python mirror imports torch here, before the
        # library is loaded, when torch is installed (dist.py needs it anyway); GBWT_HIP_NO_TORCH_PRELOAD=1 skips that.
        if "torch" not in sys.modules and not os.environ.get("GBWT_HIP_NO_TORCH_PRELOAD"):
            try:
                import torch  # noqa: F401
            except Exception:  # noqa: BLE001  (not installed, or installed and broken -- OSError / RuntimeError from its own loader: this
                pass           # library does not need it; CPU-only callers such as gbwt_hip_parse_file must not fail because of it)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


class GbwtHipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{STATUS_NAMES[status] if 0 <= status < len(STATUS_NAMES) else status}: {message}")
        self.status = status


def check(status):
    if status != OK:
        raise GbwtHipError(status, lib().gbwt_hip_last_error().decode(errors="replace"))
