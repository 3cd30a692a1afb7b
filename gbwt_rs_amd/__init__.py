"""gbwt_rs_amd -- MI355X-native (gfx950, hand-written HIP) drop-in for the GBWT LF-step hot path of
jltsiren/gbwt-rs: batched path extraction (SequenceIter) and find/extend/bidirectional search.

`api`   : host-side mirror of the reference's GBWT / GBZ interface over the C ABI (include/gbwt_hip.h)
`synth` : synthetic GBWT/GBZ generator and simple-sds writer (host only)
`csrc`  : HIP kernels + C ABI (libgbwt_hip.so)
"""
from ._lib import GFA_TRANSLATE_ALWAYS, GFA_TRANSLATE_AUTO, GFA_TRANSLATE_NEVER, MERGE_AUTO, MERGE_INSERT, MERGE_REBUILD, OPEN_ALL, OPEN_EXTRACT, OPEN_GFA, OPEN_SEARCH, REMOVE_AUTO, REMOVE_DELETE, REMOVE_REBUILD
from .api import (ALIGNMENT_DTYPE, ALIGN_NONE, ALIGN_OK, ALIGN_WIDE, BD_DTYPE, CHAIN_DTYPE, CHAIN_MATCH_DTYPE, SEED_DTYPE, STRAND_BOTH, STRAND_FORWARD, STRAND_REVERSE, FORWARD, GBWT, GBZ, FMIndex, PathFMIndex, PATHS_DEFAULT, PATHS_PAN_SN, PATHS_REF_ONLY, POS_DTYPE, REVERSE, STATE_DTYPE, GbwtHipError, decode_node, device_count, device_memory,
                  cigar_string, encode_node, encode_path, flip_node, last_suffix_array_info, parse_file, parse_gfa, reverse_complement, suffix_array_text)

__all__ = ["MERGE_AUTO", "MERGE_INSERT", "MERGE_REBUILD", "REMOVE_AUTO", "REMOVE_DELETE", "REMOVE_REBUILD", "GFA_TRANSLATE_ALWAYS", "GFA_TRANSLATE_AUTO", "GFA_TRANSLATE_NEVER", "OPEN_ALL", "OPEN_EXTRACT", "OPEN_GFA", "OPEN_SEARCH", "GBWT", "GBZ", "GbwtHipError", "FORWARD", "REVERSE", "PATHS_DEFAULT", "PATHS_PAN_SN", "PATHS_REF_ONLY", "POS_DTYPE", "STATE_DTYPE", "BD_DTYPE", "encode_node",
           "decode_node", "flip_node", "encode_path", "device_count", "device_memory", "parse_file", "parse_gfa", "suffix_array_text", "last_suffix_array_info", "FMIndex", "PathFMIndex", "SEED_DTYPE", "CHAIN_DTYPE", "CHAIN_MATCH_DTYPE", "ALIGNMENT_DTYPE", "ALIGN_OK", "ALIGN_WIDE", "ALIGN_NONE", "cigar_string", "STRAND_FORWARD", "STRAND_REVERSE", "STRAND_BOTH",
           "reverse_complement"]
