"""Host-side mirror of the reference's GBWT / GBZ interface for the hot path, batched, on MI355X.

Method names, argument meaning and None-behaviour follow the Rust API (file:line into the reference):

  GBWT.len / sequences / alphabet_size / alphabet_offset / first_node / is_bidirectional   src/gbwt.rs:108-174
  GBWT.start(ids)            GBWT::start            src/gbwt.rs:213-219
  GBWT.forward(positions)    GBWT::forward          src/gbwt.rs:222-229
  GBWT.backward(positions)   GBWT::backward         src/gbwt.rs:236-250
  GBWT.sequence(id)          GBWT::sequence         src/gbwt.rs:253-261   (None for id >= sequences)
  GBWT.sequences_csr(ids)    the batched form of sequence(): CSR arrays
  GBWT.find / extend / bd_find / extend_forward / extend_backward     src/gbwt.rs:269-367
  GBZ.path(path_id, orientation)   GBZ::path        src/gbz.rs:461-466
  GBZ.node_sequence(node_id)       GBZ::sequence    src/gbz.rs:292-298   (None for a node that does not exist)
  GBZ.path_sequences(ids, o)       gbz-extract's extract_sequence, src/bin/gbz-extract.rs:173-189 (bases of paths)
  GBWT.weakly_connected_components()   GBZ::weakly_connected_components   src/gbz.rs:570-598
  GBZ.select_paths(contig)         gbz-extract's select_paths, src/bin/gbz-extract.rs:196-264
  GBZ.tag_array(ids, sa)           gbz-extract's extract_tag_array, src/bin/gbz-extract.rs:346-371, 408-482 (tags of a suffix array)
  GBZ.suffix_array(ids) / suffix_array_text(data)   the `base`.sa and `base`.bwt that tag-array mode reads (src/bin/gbz-extract.rs:321-344, 373-406)
                                   and nothing in the reference writes: suffix array and BWT of a text, built on the device
  FMIndex.from_text(data) / GBZ.fm_index(ids)      an FM-index over such a text: count / locate / graph_positions of batches of patterns by
                                   backward search (the reference has no counterpart: what its tag array is made for)
  GBZ.reference_positions(interval)   GBZ::reference_positions   src/gbz.rs:600-657   (reference_sample_names / reference_paths: 146-196)
  GBWT.node_iter / successors / predecessors        GBZ::node_iter, successors, predecessors   src/gbz.rs:312-353 (EdgeIter 819-892)
  GBZ.node_to_segment / segment_iter / segment_successors / segment_predecessors   src/gbz.rs:370-440 (SegmentIter, LinkIter 896-1016)
  GBZ.graph_lines()                gbunzip's H-, S- and L-lines   src/bin/gbunzip.rs:193-332
  GBWT.locate / locate_csr / locate_positions      the C++ GBWT's locate(SearchState) / locate(node, i): the sequences behind a search state
                                   (the reference has no counterpart: "Locate queries" is the open box of its README's scope list)
  GBWT.from_paths / from_rows_device               the C++ GBWT's construction: the index of a set of paths, made on the device ("GBWT
                                   construction" in the same list); GBWT.records / save give the result back

Every call goes through the C ABI of libgbwt_hip.so (hand-written HIP); "not found" is reported as
None / a False entry of the validity mask, never as an exception.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import BdState, BuildInfo, Components, EdgeRows, GbwtHipError, GfaInfo, GraphText, Lines, Located, LocateInfo, Memory, OpenTimes, Paths, Pos, State, Stats, SuffixArray, SuffixArrayInfo, check

FORWARD, REVERSE = 0, 1  # support::Orientation, src/support.rs:30-47
PATHS_DEFAULT, PATHS_PAN_SN, PATHS_REF_ONLY = 0, 1, 2  # gbunzip's PathMode, src/bin/gbunzip.rs:63-76

POS_DTYPE = np.dtype([("node", "<u8"), ("offset", "<u8")])
STATE_DTYPE = np.dtype([("node", "<u8"), ("start", "<u8"), ("end", "<u8")])
BD_DTYPE = np.dtype([("forward", STATE_DTYPE), ("reverse", STATE_DTYPE)])
REFPATH_DTYPE = np.dtype([("path_id", "<u8"), ("len", "<u8"), ("first", "<u8"), ("count", "<u8")])      # gbwt_hip_reference_path
REFPOS_DTYPE = np.dtype([("offset", "<u8"), ("node", "<u8"), ("pos_offset", "<u8")])                    # gbwt_hip_reference_position
SEED_DTYPE = np.dtype([("lo", "<u8"), ("hi", "<u8"), ("start", "<u4"), ("end", "<u4"), ("strand", "<u4"), ("reserved", "<u4")])   # gbwt_hip_fm_seed
CHAIN_DTYPE = np.dtype([("text_start", "<u8"), ("text_end", "<u8"), ("read_start", "<u4"), ("read_end", "<u4"), ("score", "<u4"), ("matches", "<u4"), ("strand", "<u4"),
                        ("path", "<u4")])                                                                   # gbwt_hip_fm_chain
CHAIN_MATCH_DTYPE = np.dtype([("y", "<u8"), ("x", "<u4"), ("w", "<u4")])                                    # gbwt_hip_fm_chain_match
ALIGNMENT_DTYPE = np.dtype([("text_start", "<u8"), ("text_end", "<u8"), ("chain", "<u4"), ("edit_distance", "<u4"), ("width", "<u4"), ("status", "<u4"), ("strand", "<u4"),
                            ("path", "<u4")])                                                               # gbwt_hip_fm_alignment
ALIGN_OK, ALIGN_WIDE, ALIGN_NONE = _lib.ALIGN_OK, _lib.ALIGN_WIDE, _lib.ALIGN_NONE
_CIGAR_OPS = {1: "I", 2: "D", 7: "=", 8: "X"}


def cigar_string(ops):
    """The CIGAR of one alignment as text: `ops` are its u32 entries (length << 4) | op with BAM's codes I = 1, D = 2, '=' = 7, X = 8."""
    return "".join(f"{int(v) >> 4}{_CIGAR_OPS[int(v) & 15]}" for v in ops)
STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH = _lib.STRAND_FORWARD, _lib.STRAND_REVERSE, _lib.STRAND_BOTH

_COMPLEMENT = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    _COMPLEMENT[_a] = _b


def reverse_complement(data):
    """support::reverse_complement (src/support.rs:87-110) on the host: A/C/G/T in either case to the upper-case complement, every other byte
    to N, in reverse order; bytes in, bytes out.  FMIndex.seeds computes it on the device: this one is for callers and tests."""
    if isinstance(data, str):
        data = data.encode()
    return _COMPLEMENT[np.frombuffer(bytes(data), dtype=np.uint8)[::-1]].tobytes()


def encode_node(node_id, orientation):  # support::encode_node, src/support.rs:155-157
    return 2 * node_id + orientation


def decode_node(node):  # support::decode_node, src/support.rs:180-182
    return node // 2, node & 1


def flip_node(node):  # support::flip_node, src/support.rs:188-190
    return node ^ 1


def encode_path(path_id, orientation):  # support::encode_path, src/support.rs:229-231
    return 2 * path_id + orientation


def device_count():
    return _lib.lib().gbwt_hip_device_count()


def device_memory(device=0):
    """(free, total) bytes of a device (hipMemGetInfo)."""
    free, total = C.c_uint64(0), C.c_uint64(0)
    check(_lib.lib().gbwt_hip_device_memory(device, C.byref(free), C.byref(total)))
    return free.value, total.value


def parse_file(path):
    """Host-only parse + validation (no GPU): the statistics serialize::load_from would yield."""
    st = Stats()
    check(_lib.lib().gbwt_hip_parse_file(os.fsencode(path), C.byref(st)))
    return st


def parse_gfa(path):
    """Host-only counts of a GFA file (gbwt_hip_parse_gfa, no GPU): a dict with the fields of gbwt_hip_gfa_info."""
    g = GfaInfo()
    check(_lib.lib().gbwt_hip_parse_gfa(os.fsencode(path), C.byref(g)))
    return _as_dict(g)


def _as_dict(s, skip_reserved=False):  # the fields of a ctypes struct the library has filled, by name
    return {name: getattr(s, name) for name, _ in s._fields_ if not (skip_reserved and name == "reserved")}


def _ref_or_null(opts):  # an options struct as the library takes it: NULL = the call without options
    return C.byref(opts) if opts is not None else None


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _suffix_info(ws):  # gbwt_hip_last_suffix_array_info as a dict: the lists cut to the rounds that ran
    info = SuffixArrayInfo()
    check(_lib.lib().gbwt_hip_last_suffix_array_info(ws, C.byref(info)))
    d = _as_dict(info)
    kept = min(info.rounds + 1, 64)
    d["active"], d["round_ms"] = list(info.active[:kept]), list(info.round_ms[:kept])
    return d


def suffix_array_text(data, sentinel=0, device=0, return_bwt=False):
    """The suffix array of any bytes (gbwt_hip_suffix_array_text; no index): the permutation that orders the suffixes as unsigned byte strings
    compared to the end of the text, a proper prefix first, as a numpy uint64 array.  return_bwt: (sa, bwt uint8, runs of the bwt), with the
    byte `sentinel` in front of suffix 0."""
    text = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
    if text.ndim != 1:
        raise ValueError("data must be one-dimensional")
    sa = np.zeros(text.size, dtype=np.uint64)
    bwt = np.zeros(text.size, dtype=np.uint8) if return_bwt else None
    runs = C.c_uint64(0)
    check(_lib.lib().gbwt_hip_suffix_array_text(device, _ptr(text), text.size, int(sentinel), _ptr(sa), _ptr(bwt), C.byref(runs)))
    return (sa, bwt, runs.value) if return_bwt else sa


def last_suffix_array_info():
    """The last suffix_array_text call of the process (gbwt_hip_last_suffix_array_info without a workspace): a dict."""
    return _suffix_info(None)


def _patterns_csr(patterns):
    """Patterns as the library takes them -- (offsets uint64[m + 1], bytes uint8) -- from a list of bytes / str or from such a pair."""
    if isinstance(patterns, (bytes, bytearray, str)):
        raise TypeError("patterns must be a list of bytes / str or an (offsets, bytes) pair, not a single pattern")
    if isinstance(patterns, tuple) and len(patterns) == 2 and isinstance(patterns[0], np.ndarray):
        offsets = np.ascontiguousarray(patterns[0], dtype=np.uint64)
        data = patterns[1]
        data = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        if offsets.ndim != 1 or offsets.size == 0 or data.ndim != 1:
            raise ValueError("an (offsets, bytes) pair holds m + 1 offsets and one-dimensional bytes")
        if np.any(offsets[1:] < offsets[:-1]) or int(offsets[-1]) > data.size:
            raise ValueError("pattern offsets must ascend and end inside the bytes")
        return offsets, data
    rows = []
    for p in patterns:
        if isinstance(p, str):
            p = p.encode()
        if not isinstance(p, (bytes, bytearray)):
            raise TypeError(f"a pattern must be bytes or str, not {type(p).__name__}")
        rows.append(bytes(p))
    offsets = np.zeros(len(rows) + 1, dtype=np.uint64)
    if rows:
        np.cumsum([len(p) for p in rows], out=offsets[1:])
    return offsets, np.frombuffer(b"".join(rows), dtype=np.uint8)


class FMIndex:
    """An FM-index over a text on the device (gbwt_hip_fm_*; the reference has no counterpart): count and locate batches of patterns by backward
    search.  The order is suffix_array_text's; a pattern that does not occur has the range (0, 0), the empty one (0, n).  One thread at a time."""

    def __init__(self, handle, device=0, owner=None):
        self._L = _lib.lib()
        self._fm = handle
        self._device = device
        self._owner = owner                                # a path-level index: the GBZ it asks for tags, kept alive

    @classmethod
    def from_text(cls, data, sentinel=0, device=0, count_only=False, keep_text=False):
        """The index of any bytes (gbwt_hip_fm_build_text): the suffix array is built on the device as suffix_array_text builds it.
        count_only: no suffix array is kept, locate is refused.  keep_text: the object keeps the text as well (set_text), for alignments."""
        text = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        if text.ndim != 1:
            raise ValueError("data must be one-dimensional")
        handle = C.c_void_p()
        check(_lib.lib().gbwt_hip_fm_build_text(device, _ptr(text), text.size, int(sentinel), _lib.FM_COUNT_ONLY if count_only else 0, C.byref(handle)))
        fm = cls(handle, device)
        if keep_text:
            fm.set_text(text)
        return fm

    @classmethod
    def from_device(cls, d_text, n, sentinel=0, d_sa=None, device=0, count_only=False, stream=None):
        """gbwt_hip_fm_build_text_device: `d_text` (and `d_sa`, u64[n], or None: built by the call) are device pointers (int); only read."""
        handle = C.c_void_p()
        check(_lib.lib().gbwt_hip_fm_build_text_device(device, C.c_void_p(int(d_text)), n, int(sentinel), C.c_void_p(int(d_sa)) if d_sa else None,
                                                       _lib.FM_COUNT_ONLY if count_only else 0, stream, C.byref(handle)))
        return cls(handle, device)

    def close(self):
        if self._fm:
            self._L.gbwt_hip_fm_close(self._fm)
            self._fm = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def set_text(self, data):
        """gbwt_hip_fm_set_text: the object keeps a copy of the text it was built from in HBM, which alignments() reads.  A text of another
        length is BAD_ARGUMENT, one with another byte histogram INVALID_DATA; a second call replaces the first."""
        text = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        if text.ndim != 1:
            raise ValueError("data must be one-dimensional")
        check(self._L.gbwt_hip_fm_set_text(self._fm, _ptr(text), text.size))

    def info(self):
        """gbwt_hip_fm_info as a dict: n, sigma, block_rows, blocks, primary, index_bytes, ..., the build's phase times and the last query's."""
        info = _lib.FmIndexInfo()
        check(self._L.gbwt_hip_fm_info(self._fm, C.byref(info)))
        return _as_dict(info, skip_reserved=True)

    def count(self, patterns):
        """The SA range of every pattern: uint64[m, 2] of (lo, hi); hi - lo is the number of occurrences."""
        offsets, data = _patterns_csr(patterns)
        m = offsets.size - 1
        ranges = np.zeros((m, 2), dtype=np.uint64)
        check(self._L.gbwt_hip_fm_count(self._fm, _ptr(offsets), _ptr(data), m, _ptr(ranges)))
        return ranges

    def _rows(self, call, offsets, data):
        m = offsets.size - 1
        out = np.zeros(m + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        check(call(_ptr(offsets), _ptr(data), m, _ptr(out), None, 0, C.byref(total)))
        values = np.zeros(max(1, total.value), dtype=np.uint64)
        check(call(_ptr(offsets), _ptr(data), m, _ptr(out), _ptr(values), values.size, C.byref(total)))
        return out, values[: total.value]

    def locate_csr(self, patterns):
        """(offsets[m + 1], positions): row k holds the text positions SA[lo_k .. hi_k) of pattern k in SA order."""
        offsets, data = _patterns_csr(patterns)
        return self._rows(lambda o, b, m, *rest: self._L.gbwt_hip_fm_locate(self._fm, o, b, m, *rest), offsets, data)

    def locate(self, pattern):
        """The text positions of one pattern, in SA order."""
        return self.locate_csr([pattern])[1].copy()

    @staticmethod
    def _device_patterns(d_offsets, d_bytes, m, nbytes):
        if m < 0 or nbytes < 0:
            raise ValueError("m and the number of pattern bytes must not be negative")
        return C.c_void_p(int(d_offsets)), C.c_void_p(int(d_bytes)) if d_bytes else None, int(m), int(nbytes)

    def count_device(self, d_offsets, d_bytes, m, nbytes):
        """gbwt_hip_fm_count_device: the CSR of m patterns (u64 offsets, `nbytes` bytes) behind device pointers (int); a _lib.FmLocated whose
        d_ranges[2 m] stays in HBM until the next request."""
        out = _lib.FmLocated()
        check(self._L.gbwt_hip_fm_count_device(self._fm, *self._device_patterns(d_offsets, d_bytes, m, nbytes), C.byref(out)))
        return out

    def locate_device(self, d_offsets, d_bytes, m, nbytes):
        """gbwt_hip_fm_locate_device: d_offsets[m + 1], d_values[total] (positions) and d_ranges[2 m] in HBM until the next request."""
        out = _lib.FmLocated()
        check(self._L.gbwt_hip_fm_locate_device(self._fm, *self._device_patterns(d_offsets, d_bytes, m, nbytes), C.byref(out)))
        return out

    @staticmethod
    def _seed_options(min_length, strands, max_occurrences):
        if strands not in (STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH):
            raise ValueError("strands must be STRAND_FORWARD, STRAND_REVERSE or STRAND_BOTH")
        if int(min_length) < 0 or int(max_occurrences) < 0:
            raise ValueError("min_length and max_occurrences must not be negative")
        return _lib.FmSeedOptions(int(min_length), int(strands), int(max_occurrences), 0, 0)

    def _seed_rows(self, call, offsets, data, opts):  # the size query, then the fill, which only copies
        m = offsets.size - 1
        read_offsets = np.zeros(m + 1, dtype=np.uint64)
        n_seeds, n_hits = C.c_uint64(0), C.c_uint64(0)
        reads = (_ptr(offsets), _ptr(data), m, C.byref(opts), _ptr(read_offsets))
        check(call(*reads, None, 0, C.byref(n_seeds), None, None, 0, C.byref(n_hits)))
        with_hits = opts.max_occurrences != 0
        seeds = np.zeros(max(1, n_seeds.value), dtype=SEED_DTYPE)
        hit_offsets = np.zeros(n_seeds.value + 1, dtype=np.uint64) if with_hits else None
        hits = np.zeros(max(1, n_hits.value), dtype=np.uint64) if with_hits else None
        check(call(*reads, seeds.ctypes.data, seeds.size, C.byref(n_seeds), _ptr(hit_offsets), _ptr(hits), hits.size if with_hits else 0, C.byref(n_hits)))
        return read_offsets, seeds[: n_seeds.value], hit_offsets, hits[: n_hits.value] if with_hits else None

    def seeds(self, reads, min_length=1, strands=STRAND_BOTH, max_occurrences=0):
        """The maximal exact matches of every read (gbwt_hip_fm_seeds): (read_offsets[m + 1], seeds, hit_offsets, hits).  `reads` as the
        patterns of count; `seeds` is a structured array of SEED_DTYPE -- start, end, strand and the SA range (lo, hi) of read[start:end] on
        that strand --, row k of it the seeds of read k, forward strand first, starts and ends ascending; the reverse strand is
        reverse_complement(read), computed on the device, and its seeds are in its coordinates.  max_occurrences > 0: row i of (hit_offsets,
        hits) holds the text positions SA[lo:hi] of seed i, empty where it occurs more often; else both are None."""
        offsets, data = _patterns_csr(reads)
        opts = self._seed_options(min_length, strands, max_occurrences)
        return self._seed_rows(lambda *a: self._L.gbwt_hip_fm_seeds(self._fm, *a), offsets, data, opts)

    def seeds_device(self, d_offsets, d_bytes, m, nbytes, min_length=1, strands=STRAND_BOTH, max_occurrences=0):
        """gbwt_hip_fm_seeds_device: a _lib.FmSeedRows whose d_read_offsets[m + 1], d_seeds[total_seeds] and -- with hits -- d_hit_offsets[total_seeds + 1],
        d_hits[total_hits] stay in HBM until the next seeds request."""
        out = _lib.FmSeedRows()
        opts = self._seed_options(min_length, strands, max_occurrences)
        check(self._L.gbwt_hip_fm_seeds_device(self._fm, *self._device_patterns(d_offsets, d_bytes, m, nbytes), C.byref(opts), C.byref(out)))
        return out

    def last_seed_info(self):
        """gbwt_hip_fm_last_seed_info as a dict: stride, reads, anchors, refined_ends, steps, idle_share, seeds, hits, over_max, scratch bytes, phase times."""
        info = _lib.FmSeedInfo()
        check(self._L.gbwt_hip_fm_last_seed_info(self._fm, C.byref(info)))
        return _as_dict(info, skip_reserved=True)

    @staticmethod
    def _chain_options(max_gap, max_skew, gap_cost, min_score, max_matches):
        values = [int(v) for v in (max_gap, max_skew, gap_cost, min_score, max_matches)]
        if any(v < 0 for v in values) or any(v >= 1 << 32 for v in values[:4]):
            raise ValueError("max_gap, max_skew, gap_cost and min_score are 32-bit counts, max_matches a count")
        return _lib.FmChainOptions(*values, 0, 0)

    def chains(self, reads, min_length=1, strands=STRAND_BOTH, max_occurrences=1000, max_gap=0, max_skew=0, gap_cost=1, min_score=1, max_matches=0):
        """The colinear chains of every read's hits (gbwt_hip_fm_chains): (read_offsets[m + 1], chains, match_offsets, matches).  The seeds are
        those of seeds(reads, min_length, strands, max_occurrences) with hits; every hit of a seed is a match (y text position, x start in
        the read, w length).  `chains` is a structured array of CHAIN_DTYPE, row k of it the chains of read k: those of the forward strand,
        then those of the reverse strand (in the coordinates of reverse_complement(read)), each strand best first; row c of (match_offsets,
        matches) holds the members of chain c, a CHAIN_MATCH_DTYPE array ascending by (y, x).  max_gap / max_skew 0: 5000 / 500; max_matches:
        a (read, strand) with more matches yields no chains (0: no limit).  `path` of a chain is 0 on an index of a plain text."""
        offsets, data = _patterns_csr(reads)
        seed_opts = self._seed_options(min_length, strands, max_occurrences)
        chain_opts = self._chain_options(max_gap, max_skew, gap_cost, min_score, max_matches)
        m = offsets.size - 1
        read_offsets = np.zeros(m + 1, dtype=np.uint64)
        n_chains, n_matches = C.c_uint64(0), C.c_uint64(0)
        request = (self._fm, _ptr(offsets), _ptr(data), m, C.byref(seed_opts), C.byref(chain_opts), _ptr(read_offsets))
        check(self._L.gbwt_hip_fm_chains(*request, None, 0, C.byref(n_chains), None, None, 0, C.byref(n_matches)))   # the size query computes, the fill only copies
        chains = np.zeros(max(1, n_chains.value), dtype=CHAIN_DTYPE)
        match_offsets = np.zeros(n_chains.value + 1, dtype=np.uint64)
        matches = np.zeros(max(1, n_matches.value), dtype=CHAIN_MATCH_DTYPE)
        check(self._L.gbwt_hip_fm_chains(*request, chains.ctypes.data, chains.size, C.byref(n_chains), _ptr(match_offsets), matches.ctypes.data, matches.size, C.byref(n_matches)))
        return read_offsets, chains[: n_chains.value], match_offsets, matches[: n_matches.value]

    def chains_device(self, d_offsets, d_bytes, m, nbytes, min_length=1, strands=STRAND_BOTH, max_occurrences=1000, max_gap=0, max_skew=0, gap_cost=1, min_score=1, max_matches=0):
        """gbwt_hip_fm_chains_device: a _lib.FmChainRows whose d_read_offsets[m + 1], d_chains[total_chains], d_match_offsets[total_chains + 1] and
        d_matches[total_matches] stay in HBM until the next chains request."""
        out = _lib.FmChainRows()
        seed_opts = self._seed_options(min_length, strands, max_occurrences)
        chain_opts = self._chain_options(max_gap, max_skew, gap_cost, min_score, max_matches)
        check(self._L.gbwt_hip_fm_chains_device(self._fm, *self._device_patterns(d_offsets, d_bytes, m, nbytes), C.byref(seed_opts), C.byref(chain_opts), C.byref(out)))
        return out

    def last_chain_info(self):
        """gbwt_hip_fm_last_chain_info as a dict: items, matches, skipped_items, pairs, chains, chain_matches, tile_matches, scratch bytes, phase times."""
        info = _lib.FmChainInfo()
        check(self._L.gbwt_hip_fm_last_chain_info(self._fm, C.byref(info)))
        return _as_dict(info)

    @staticmethod
    def _align_options(band, max_width, max_alignments):
        values = [int(v) for v in (band, max_width, max_alignments)]
        if any(v < 0 for v in values) or any(v >= 1 << 32 for v in values[:2]):
            raise ValueError("band and max_width are 32-bit counts, max_alignments a count")
        return _lib.FmAlignOptions(*values, 0, 0)

    def alignments(self, reads, min_length=1, strands=STRAND_BOTH, max_occurrences=1000, max_gap=0, max_skew=0, gap_cost=1, min_score=1, max_matches=0, band=16, max_width=0,
                   max_alignments=0):
        """The alignments of every read's chains (gbwt_hip_fm_alignments): (read_offsets[m + 1], alignments, cigar_offsets, cigars).  The
        chains are those of chains(reads, <the same seed and chain keywords>); per (read, strand) the first max_alignments of them (0: all) are
        aligned to the kept text (set_text, from_text(keep_text=True), PathFMIndex.keep_text) by a banded edit distance: `band` diagonals
        on either side of the chain's own, at most max_width (0: 256) in all.  `alignments` is a structured array of ALIGNMENT_DTYPE -- status
        ALIGN_OK, ALIGN_WIDE (the band is wider than max_width) or ALIGN_NONE (no end inside the band) --, row k of it the alignments of read k,
        forward strand first, in chain order; row a of (cigar_offsets, cigars) holds the CIGAR of alignment a as u32 entries (cigar_string)."""
        offsets, data = _patterns_csr(reads)
        seed_opts = self._seed_options(min_length, strands, max_occurrences)
        chain_opts = self._chain_options(max_gap, max_skew, gap_cost, min_score, max_matches)
        align_opts = self._align_options(band, max_width, max_alignments)
        m = offsets.size - 1
        read_offsets = np.zeros(m + 1, dtype=np.uint64)
        n_alignments, n_cigars = C.c_uint64(0), C.c_uint64(0)
        request = (self._fm, _ptr(offsets), _ptr(data), m, C.byref(seed_opts), C.byref(chain_opts), C.byref(align_opts), _ptr(read_offsets))
        check(self._L.gbwt_hip_fm_alignments(*request, None, 0, C.byref(n_alignments), None, None, 0, C.byref(n_cigars)))   # the size query computes, the fill only copies
        alignments = np.zeros(max(1, n_alignments.value), dtype=ALIGNMENT_DTYPE)
        cigar_offsets = np.zeros(n_alignments.value + 1, dtype=np.uint64)
        cigars = np.zeros(max(1, n_cigars.value), dtype=np.uint32)
        check(self._L.gbwt_hip_fm_alignments(*request, alignments.ctypes.data, alignments.size, C.byref(n_alignments), _ptr(cigar_offsets), cigars.ctypes.data, cigars.size,
                                             C.byref(n_cigars)))
        return read_offsets, alignments[: n_alignments.value], cigar_offsets, cigars[: n_cigars.value]

    def alignments_device(self, d_offsets, d_bytes, m, nbytes, min_length=1, strands=STRAND_BOTH, max_occurrences=1000, max_gap=0, max_skew=0, gap_cost=1, min_score=1, max_matches=0,
                          band=16, max_width=0, max_alignments=0):
        """gbwt_hip_fm_alignments_device: a _lib.FmAlignmentRows whose d_read_offsets[m + 1], d_alignments[total_alignments],
        d_cigar_offsets[total_alignments + 1] and d_cigars[total_cigars] stay in HBM until the next alignments request."""
        out = _lib.FmAlignmentRows()
        seed_opts = self._seed_options(min_length, strands, max_occurrences)
        chain_opts = self._chain_options(max_gap, max_skew, gap_cost, min_score, max_matches)
        align_opts = self._align_options(band, max_width, max_alignments)
        check(self._L.gbwt_hip_fm_alignments_device(self._fm, *self._device_patterns(d_offsets, d_bytes, m, nbytes), C.byref(seed_opts), C.byref(chain_opts), C.byref(align_opts),
                                                    C.byref(out)))
        return out

    def last_align_info(self):
        """gbwt_hip_fm_last_align_info as a dict: items, chains, alignments, wide, unreachable, cells, cigar_ops, lds_alignments,
        global_alignments, tile_bytes, text_bytes, scratch bytes, phase times."""
        info = _lib.FmAlignInfo()
        check(self._L.gbwt_hip_fm_last_align_info(self._fm, C.byref(info)))
        return _as_dict(info, skip_reserved=True)


class PathFMIndex(FMIndex):
    """The FM-index of the text of paths of a GBZ (GBZ.fm_index): FMIndex, and the graph positions of the occurrences."""

    def keep_text(self):
        """gbwt_hip_fm_keep_path_text: the object keeps the text of its paths -- asked of the bases family again and copied on the device --,
        which alignments() reads."""
        g = self._owner
        check(self._L.gbwt_hip_fm_keep_path_text(self._fm, g._h, g._ws))

    def graph_positions_csr(self, patterns, unique=False):
        """(offsets[m + 1], tags): row k holds the tags -- ((node << 11) | (orientation << 10)) + offset, 0 on an endmarker -- of the first
        bases of pattern k's occurrences in SA order, or with unique=True the distinct tags ascending."""
        offsets, data = _patterns_csr(patterns)
        g = self._owner
        return self._rows(lambda o, b, m, *rest: self._L.gbwt_hip_fm_graph_positions(self._fm, g._h, g._ws, o, b, m, int(bool(unique)), *rest), offsets, data)

    def graph_positions(self, pattern, unique=True):
        return self.graph_positions_csr([pattern], unique)[1].copy()

    def graph_positions_device(self, d_offsets, d_bytes, m, nbytes, unique=False):
        """gbwt_hip_fm_graph_positions_device: as locate_device, with tags in d_values."""
        out = _lib.FmLocated()
        g = self._owner
        check(self._L.gbwt_hip_fm_graph_positions_device(self._fm, g._h, g._ws, *self._device_patterns(d_offsets, d_bytes, m, nbytes), int(bool(unique)), C.byref(out)))
        return out

    def seeds(self, reads, min_length=1, strands=STRAND_BOTH, max_occurrences=0, graph=False):
        """FMIndex.seeds; graph=True (with max_occurrences > 0): the hits are the tags of the occurrences' first bases, as graph_positions_csr
        gives them with unique=False (gbwt_hip_fm_seed_graph_positions)."""
        if not graph:
            return super().seeds(reads, min_length, strands, max_occurrences)
        offsets, data = _patterns_csr(reads)
        opts = self._seed_options(min_length, strands, max_occurrences)
        g = self._owner
        return self._seed_rows(lambda *a: self._L.gbwt_hip_fm_seed_graph_positions(self._fm, g._h, g._ws, *a), offsets, data, opts)

    def seeds_device(self, d_offsets, d_bytes, m, nbytes, min_length=1, strands=STRAND_BOTH, max_occurrences=0, graph=False):
        """FMIndex.seeds_device; graph=True: tags in d_hits (gbwt_hip_fm_seed_graph_positions_device)."""
        if not graph:
            return super().seeds_device(d_offsets, d_bytes, m, nbytes, min_length, strands, max_occurrences)
        out = _lib.FmSeedRows()
        opts = self._seed_options(min_length, strands, max_occurrences)
        g = self._owner
        check(self._L.gbwt_hip_fm_seed_graph_positions_device(self._fm, g._h, g._ws, *self._device_patterns(d_offsets, d_bytes, m, nbytes), C.byref(opts), C.byref(out)))
        return out


class GBWT:
    """A GBWT index resident in HBM.  Mirrors gbwt::GBWT (src/gbwt.rs:95-385) for the hot path."""

    def __init__(self, handle, owner=None, device=0):
        self._L = _lib.lib()
        self._h = handle
        self._device = device
        self._owner = owner                 # a view of another object's index (another_workspace): that object closes it
        self._ws = C.c_void_p()
        check(self._L.gbwt_hip_workspace_create(self._h, C.byref(self._ws)))
        self._stats = Stats()
        check(self._L.gbwt_hip_get_stats(self._h, C.byref(self._stats)))

    # ---- construction -------------------------------------------------------------------------
    @classmethod
    def load(cls, path, device=0, flags=_lib.OPEN_ALL):
        """serialize::load_from::<GBWT | GBZ>(path) (src/gbwt.rs:402-438, src/gbz.rs:674-717).  flags: what the handle is for
        (_lib.OPEN_EXTRACT | OPEN_SEARCH | OPEN_GFA, gbwt_hip_open_file_flags): only those structures are built in HBM."""
        h = C.c_void_p()
        check(_lib.lib().gbwt_hip_open_file_flags(os.fsencode(path), device, flags, C.byref(h)))
        return cls(h, device=device)

    @classmethod
    def from_records(cls, data, starts, alphabet_offset, alphabet_size, sequences, size, bidirectional=True, device=0, flags=_lib.OPEN_ALL):
        """From the raw record stream of a bwt::BWT (compressed_record, src/bwt.rs:134-143) + header fields."""
        d = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        s = np.ascontiguousarray(starts, dtype=np.uint64)
        h = C.c_void_p()
        check(_lib.lib().gbwt_hip_open_records_flags(_ptr(d), d.size, _ptr(s), s.size, alphabet_offset, alphabet_size,
                                                     sequences, size, int(bidirectional), device, flags, C.byref(h)))
        return cls(h, device=device)

    @staticmethod
    def _path_set(paths):
        """(offsets u64[n + 1], nodes u64) of a list of paths; every path one-dimensional, of integers, none of them negative."""
        rows = []
        for k, p in enumerate(paths):
            a = np.asarray(p)
            if a.ndim != 1:
                raise ValueError(f"path {k} is not one-dimensional")
            if a.size and a.dtype.kind not in "iu":
                raise TypeError(f"path {k} does not hold integers")
            if a.size and a.dtype.kind == "i" and int(a.min()) < 0:
                raise ValueError(f"path {k} holds a negative node")
            rows.append(a.astype(np.uint64))
        offsets = np.zeros(len(rows) + 1, dtype=np.uint64)
        if rows:
            np.cumsum([r.size for r in rows], out=offsets[1:])
        nodes = np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint64)
        return offsets, np.ascontiguousarray(nodes, dtype=np.uint64)

    @classmethod
    def from_paths(cls, paths, bidirectional=True, device=0, flags=_lib.OPEN_ALL):
        """The GBWT of a set of paths, constructed on the device (gbwt_hip_build_from_paths).  paths: a list of lists or numpy arrays of
        GBWT-encoded nodes (2 * id + orientation, id >= 1); bidirectional: sequence 2p is path p, sequence 2p + 1 its reverse."""
        offsets, nodes = cls._path_set(paths)
        h = C.c_void_p()
        check(_lib.lib().gbwt_hip_build_from_paths(offsets.ctypes.data, _ptr(nodes), offsets.size - 1, int(bool(bidirectional)), device, flags, C.byref(h)))
        return cls(h, device=device)

    @classmethod
    def from_rows_device(cls, paths_struct, n, bidirectional=True, device=0, flags=_lib.OPEN_ALL):
        """The same for the first n rows of a device-resident extraction (the Paths struct of extract_device): the rows are only read."""
        if not isinstance(paths_struct, Paths):
            raise TypeError("from_rows_device takes the Paths struct of extract_device")
        if n < 0 or n > paths_struct.n:
            raise ValueError(f"n = {n} rows of a struct that holds {paths_struct.n}")
        h = C.c_void_p()
        check(_lib.lib().gbwt_hip_build_from_rows_device(paths_struct.d_offsets, paths_struct.d_nodes, n, int(bool(bidirectional)), device, flags, C.byref(h)))
        return cls(h, device=device)

    @classmethod
    def merge(cls, a, b=None, algorithm=None, device=None, flags=_lib.OPEN_ALL):
        """The index of a's sequences followed by b's, merged on the device (gbwt_hip_merge): what from_paths gives for the paths of a, then
        those of b, with the metadata, tags and -- for two GBZ -- node labels of both.  algorithm: None (the library chooses: the
        rebuild where both inputs are open for extraction, else the insertion) or _lib.MERGE_AUTO | MERGE_REBUILD | MERGE_INSERT.  a may be a list of handles (b None): more than two fold left.  The inputs are
        only read.  device: None, or the device the inputs are on."""
        handles = list(a) if b is None else [a, b]
        if len(handles) < 2:
            raise ValueError("merge takes two handles, or a list of at least two")
        for x in handles:
            if not isinstance(x, GBWT) or not getattr(x, "_h", None):
                raise TypeError("merge takes open GBWT / GBZ handles")
            if device is not None and x._device != device:
                raise ValueError(f"a handle is on device {x._device}, not on {device}")
        opts = None if algorithm is None else _lib.MergeOptions(int(algorithm), 0)
        result = None
        for k, nxt in enumerate(handles[1:]):
            left = handles[0] if result is None else result
            h = C.c_void_p()
            check(_lib.lib().gbwt_hip_merge(left._h, nxt._h, _ref_or_null(opts), flags if k == len(handles) - 2 else _lib.OPEN_ALL, C.byref(h)))
            merged = cls(h, device=left._device)
            if result is not None:
                result.close()
            result = merged
        return result

    def last_merge_info(self):
        """The merge behind the handle (gbwt_hip_last_merge_info): a dict; all zeros for a handle that was not merged."""
        m = _lib.MergeInfo()
        check(self._L.gbwt_hip_last_merge_info(self._h, C.byref(m)))
        return _as_dict(m)

    def remove_paths(self, path_ids, algorithm=None, flags=_lib.OPEN_ALL):
        """The index without the paths path_ids, a new handle of the same class (gbwt_hip_remove_paths): what from_paths gives for the kept
        sequences in their old order, with the metadata, tags and -- for a GBZ -- node labels that still apply.  In a bidirectional index
        path p is the sequences 2p and 2p + 1.  algorithm: None (the library chooses: the rebuild where the handle is open for
        extraction, else the deletion) or _lib.REMOVE_AUTO | REMOVE_REBUILD | REMOVE_DELETE.  This handle is only read."""
        ids = np.ascontiguousarray(np.asarray(path_ids, dtype=np.int64).reshape(-1))
        if ids.size and int(ids.min()) < 0:
            raise ValueError("a path id is negative")
        ids = ids.astype(np.uint64)
        opts = None if algorithm is None else _lib.RemoveOptions(int(algorithm), 0)
        h = C.c_void_p()
        check(self._L.gbwt_hip_remove_paths(self._h, _ptr(ids), ids.size, _ref_or_null(opts), flags, C.byref(h)))
        return type(self)(h, device=self._device)

    def keep_paths(self, path_ids, algorithm=None, flags=_lib.OPEN_ALL):
        """The index of the paths path_ids alone, in their old order: remove_paths of the complement."""
        total = self.sequences() // 2 if self.is_bidirectional() else self.sequences()
        keep = np.zeros(total, dtype=bool)
        ids = np.asarray(path_ids, dtype=np.int64).reshape(-1)
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= total):
            raise ValueError(f"a path id is not in [0, {total})")
        keep[ids] = True
        return self.remove_paths(np.flatnonzero(~keep), algorithm=algorithm, flags=flags)

    def last_remove_info(self):
        """The removal behind the handle (gbwt_hip_last_remove_info): a dict; all zeros for a handle that did not come from a removal."""
        m = _lib.RemoveInfo()
        check(self._L.gbwt_hip_last_remove_info(self._h, C.byref(m)))
        return _as_dict(m)

    def records(self):
        """(data u8[], starts u64[records]) of the handle: its record stream and dense record starts (gbwt_hip_records)."""
        data_len, records = C.c_uint64(0), C.c_uint64(0)
        check(self._L.gbwt_hip_records(self._h, None, 0, C.byref(data_len), None, 0, C.byref(records)))
        data, starts = np.zeros(data_len.value, dtype=np.uint8), np.zeros(records.value, dtype=np.uint64)
        check(self._L.gbwt_hip_records(self._h, _ptr(data), data.size, C.byref(data_len), _ptr(starts), starts.size, C.byref(records)))
        return data, starts

    def save(self, path):
        """Writes the index in the simple-sds format (gbwt_hip_save): a GBZ handle as a GBZ v1 container, a GBWT handle as a GBWT file."""
        check(self._L.gbwt_hip_save(self._h, os.fsencode(path)))

    def last_build_info(self):
        """The construction behind the handle (gbwt_hip_last_build_info): a dict; all zeros for a handle that was not built."""
        b = BuildInfo()
        check(self._L.gbwt_hip_last_build_info(self._h, C.byref(b)))
        return _as_dict(b)

    def close(self):
        if getattr(self, "_ws", None):
            self._L.gbwt_hip_workspace_destroy(self._ws)
            self._ws = None
        if getattr(self, "_h", None):
            if getattr(self, "_owner", None) is None:
                self._L.gbwt_hip_close(self._h)
            self._h = None
            self._owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def another_workspace(self):
        """The same index through a workspace of its own: what a second host thread uses (a handle is immutable after open and safe
        for concurrent read-only calls as long as every thread has its own workspace; the reference shares &GBZ across rayon
        workers, src/bin/gbunzip.rs:421-434).  The view keeps this object alive and never closes the index."""
        return type(self)(self._h, owner=self, device=self._device)

    def new_workspace(self):
        """A fresh workspace: the GBWT_HIP_* extraction knobs are read when a workspace is created, not per call."""
        if getattr(self, "_ws", None):
            self._L.gbwt_hip_workspace_destroy(self._ws)
        self._ws = C.c_void_p()
        check(self._L.gbwt_hip_workspace_create(self._h, C.byref(self._ws)))

    def open_times(self):
        """Where the time of the open went (gbwt_hip_get_open_times): a dict of milliseconds and counts."""
        t = OpenTimes()
        check(self._L.gbwt_hip_get_open_times(self._h, C.byref(t)))
        return _as_dict(t)

    def memory_usage(self):
        """Bytes held by the index (device, host) and by this object's workspace (gbwt_hip_memory_usage): a dict."""
        m = Memory()
        check(self._L.gbwt_hip_memory_usage(self._h, self._ws, C.byref(m)))
        return _as_dict(m)

    # ---- statistics (src/gbwt.rs:105-175) -----------------------------------------------------
    def len(self):
        return self._stats.size

    def is_empty(self):
        return self.len() == 0

    def sequences(self):
        return self._stats.sequences

    def alphabet_size(self):
        return self._stats.alphabet_size

    def alphabet_offset(self):
        return self._stats.alphabet_offset

    def effective_size(self):
        return self.alphabet_size() - self.alphabet_offset()

    def first_node(self):
        return self.alphabet_offset() + 1

    def has_node(self, node):
        return self.alphabet_offset() < node < self.alphabet_size()

    def is_bidirectional(self):
        return bool(self._stats.bidirectional)

    def has_metadata(self):
        return bool(self._stats.has_metadata)

    @property
    def stats(self):
        return self._stats

    # ---- navigation ---------------------------------------------------------------------------
    def start(self, ids):
        """GBWT::start for an array of sequence ids -> (positions[POS_DTYPE], valid[bool])."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        out = np.zeros(ids.size, dtype=POS_DTYPE)
        valid = np.zeros(ids.size, dtype=np.uint8)
        check(self._L.gbwt_hip_start(self._h, self._ws, _ptr(ids), ids.size, _ptr(out), _ptr(valid)))
        return out, valid.astype(bool)

    def forward(self, positions):
        """GBWT::forward for an array of positions -> (positions, valid)."""
        pos = np.ascontiguousarray(positions, dtype=POS_DTYPE)
        out = np.zeros(pos.size, dtype=POS_DTYPE)
        valid = np.zeros(pos.size, dtype=np.uint8)
        check(self._L.gbwt_hip_forward(self._h, self._ws, _ptr(pos), pos.size, _ptr(out), _ptr(valid)))
        return out, valid.astype(bool)

    def backward(self, positions):
        """GBWT::backward (src/gbwt.rs:236-250) for an array of positions -> (positions, valid)."""
        pos = np.ascontiguousarray(positions, dtype=POS_DTYPE)
        out = np.zeros(pos.size, dtype=POS_DTYPE)
        valid = np.zeros(pos.size, dtype=np.uint8)
        check(self._L.gbwt_hip_backward(self._h, self._ws, _ptr(pos), pos.size, _ptr(out), _ptr(valid)))
        return out, valid.astype(bool)

    def sequences_csr(self, ids, return_valid=False):
        """GBWT::sequence(id).collect() for every id -> (offsets[u64, n+1], nodes[u32]) [, valid[bool]].

        One walk of the sequences: they are extracted into HBM, the host array is sized from the result and filled by a
        copy.  An id >= sequences() -- GBWT::sequence returns None, src/gbwt.rs:254-256 -- gets an empty row and
        valid[k] = False; it never fails the batch."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        out = self.extract_device(ids)
        offsets = np.zeros(ids.size + 1, dtype=np.uint64)
        nodes = np.empty(max(1, out.total), dtype=np.uint32)
        check(self._L.gbwt_hip_copy_result(self._h, self._ws, _ptr(offsets), _ptr(nodes) if out.total else None, nodes.size))
        if return_valid:
            return offsets, nodes[: out.total], ids < np.uint64(self.sequences())
        return offsets, nodes[: out.total]

    def sequence(self, seq_id):
        """GBWT::sequence(id): list of GBWT nodes, or None if there is no such sequence."""
        if seq_id >= self.sequences():
            return None
        offsets, nodes = self.sequences_csr([seq_id])
        return [int(x) for x in nodes]

    def extract_device(self, ids):
        """Device-resident extraction (what bench.py times): returns a Paths struct with device pointers."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        out = Paths()
        check(self._L.gbwt_hip_extract_device(self._h, self._ws, _ptr(ids), ids.size, C.byref(out)))
        return out

    def extract_part_device(self, ids, part, parts):
        """Stretch `part` of `parts` of every row (gbwt_hip_extract_part_device): the rows are cut at sequence samples, the stretches of a
        row back to back are the row.  What one rank of `parts` extracts (dist.Comm.gather_rows(..., layout=GATHER_PARTS) joins them)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        out = Paths()
        check(self._L.gbwt_hip_extract_part_device(self._h, self._ws, _ptr(ids), ids.size, part, parts, C.byref(out)))
        return out

    def part_csr(self, ids, part, parts):
        """extract_part_device + copy: (offsets[u64, n + 1], nodes[u32]) of the stretches."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        out = self.extract_part_device(ids, part, parts)
        offsets = np.zeros(ids.size + 1, dtype=np.uint64)
        nodes = np.empty(max(1, out.total), dtype=np.uint32)
        check(self._L.gbwt_hip_copy_result(self._h, self._ws, _ptr(offsets), _ptr(nodes) if out.total else None, nodes.size))
        return offsets, nodes[: out.total]

    def last_offsets(self, n):
        """The row offsets (u64[n + 1]) of the last extract_device() / extract_part_device() of n rows."""
        offsets = np.zeros(n + 1, dtype=np.uint64)
        check(self._L.gbwt_hip_copy_result(self._h, self._ws, _ptr(offsets), None, 0))
        return offsets

    def path_sums(self, n):
        """Per-path sums of node ids of the last extract_device() (device-side reduction)."""
        out = np.zeros(n, dtype=np.uint64)
        check(self._L.gbwt_hip_path_sums(self._h, self._ws, _ptr(out), n))
        return out

    def path_hashes(self, n):
        """Per-path ORDER-dependent checksums of the last extract_device(): sum of (node + 1) * splitmix64(position), gbwt_hip.h."""
        out = np.zeros(n, dtype=np.uint64)
        check(self._L.gbwt_hip_path_hashes(self._h, self._ws, _ptr(out), n))
        return out

    def copy_path(self, k):
        """Row k of the last extract_device() as a host array."""
        ln = C.c_uint64(0)
        check(self._L.gbwt_hip_copy_path(self._h, self._ws, k, None, 0, C.byref(ln)))
        out = np.zeros(max(1, ln.value), dtype=np.uint32)
        check(self._L.gbwt_hip_copy_path(self._h, self._ws, k, _ptr(out), out.size, C.byref(ln)))
        return out[: ln.value]

    def last_kernel_ms(self):
        walk, total = C.c_float(0), C.c_float(0)
        check(self._L.gbwt_hip_last_kernel_ms(self._ws, C.byref(walk), C.byref(total)))
        return walk.value, total.value

    def last_query_ms(self):
        """Kernel time (HIP events) of the last start / forward / backward / find / extend / search / follow call."""
        ms = C.c_float(0)
        check(self._L.gbwt_hip_last_query_ms(self._ws, C.byref(ms)))
        return ms.value

    def tune(self, walk_mode=0, paths_per_wave=0, small_record=16):
        """Kernel tuning knobs of gbwt_hip_workspace_tune (results never depend on them)."""
        check(self._L.gbwt_hip_workspace_tune(self._ws, walk_mode, paths_per_wave, small_record))

    def stream(self):
        return self._L.gbwt_hip_workspace_stream(self._ws)

    # ---- graph topology -----------------------------------------------------------------------
    def components_device(self):
        """The weakly connected components as they lie in HBM (gbwt_hip_components_device): a Components struct -- d_component[slots] (slot s =
        node id min_node + s; 0xFFFFFFFF for a node that does not exist), the CSR d_offsets[components + 1] / d_nodes[nodes], d_path_component[paths]
        and the counts.  Made by the first call on the handle, valid while it is open."""
        out = Components()
        check(self._L.gbwt_hip_components_device(self._h, C.byref(out)))
        return out

    def components_csr(self):
        """GBZ::weakly_connected_components (src/gbz.rs:570-598) as CSR: (offsets[u64, components + 1], node ids[u64]); the components in order of
        their smallest node id, the nodes ascending inside."""
        components, nodes = C.c_uint64(0), C.c_uint64(0)
        check(self._L.gbwt_hip_weakly_connected_components(self._h, None, 0, None, 0, C.byref(components), C.byref(nodes)))
        offsets = np.zeros(components.value + 1, dtype=np.uint64)
        ids = np.zeros(max(1, nodes.value), dtype=np.uint64)
        check(self._L.gbwt_hip_weakly_connected_components(self._h, _ptr(offsets), offsets.size, _ptr(ids), ids.size, C.byref(components), C.byref(nodes)))
        return offsets, ids[: nodes.value]

    def weakly_connected_components(self):
        """GBZ::weakly_connected_components: a list of numpy arrays of node ids, in the reference's order."""
        offsets, ids = self.components_csr()
        return [ids[int(offsets[c]):int(offsets[c + 1])] for c in range(offsets.size - 1)]

    def path_components(self, path_ids):
        """The component of the first node of every path (uint32; 0xFFFFFFFF for an empty path): what select_paths looks up
        (src/bin/gbz-extract.rs:243-246).  GbwtHipError(BAD_ARGUMENT) for an id that is no path."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        if ids.ndim != 1:
            raise ValueError("path_ids must be one-dimensional")
        out = np.zeros(ids.size, dtype=np.uint32)
        check(self._L.gbwt_hip_path_components(self._h, _ptr(ids), ids.size, _ptr(out)))
        return out

    def last_components_ms(self):
        """HIP-event time of the build that made the components of this handle and its launches (gbwt_hip_last_components_ms): a dict with
        hook_ms, jump_ms, shape_ms, hook_launches, jump_launches, shape_launches."""
        t = _lib.ComponentsTimes()
        check(self._L.gbwt_hip_last_components_ms(self._h, C.byref(t)))
        return _as_dict(t)

    # ---- the graph: nodes and edges (any handle) --------------------------------------------------
    def node_iter(self):
        """GBZ::node_iter (src/gbz.rs:312-317): the ids of the nodes that exist (GBZ::has_node), ascending, as a numpy uint64 array."""
        total = C.c_uint64(0)
        check(self._L.gbwt_hip_node_ids(self._h, None, 0, C.byref(total)))
        out = np.zeros(max(1, total.value), dtype=np.uint64)
        check(self._L.gbwt_hip_node_ids(self._h, _ptr(out), out.size, C.byref(total)))
        return out[: total.value]

    @staticmethod
    def _queries(ids, orientations):
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        orient = np.ascontiguousarray(np.broadcast_to(np.asarray(orientations), ids.shape), dtype=np.uint8)
        if ids.ndim != 1:
            raise ValueError("ids must be one-dimensional")
        return ids, orient

    def _rows_csr(self, fn, ids, orientations, predecessors):
        ids, orient = self._queries(ids, orientations)
        offsets = np.zeros(ids.size + 1, dtype=np.uint64)
        valid = np.zeros(ids.size, dtype=np.uint8)
        total = C.c_uint64(0)
        check(fn(self._h, self._ws, _ptr(ids), _ptr(orient), ids.size, int(bool(predecessors)), _ptr(offsets), None, 0, C.byref(total), _ptr(valid)))
        out = np.zeros(max(1, total.value), dtype=np.uint64)
        check(fn(self._h, self._ws, _ptr(ids), _ptr(orient), ids.size, int(bool(predecessors)), _ptr(offsets), _ptr(out), out.size, C.byref(total), _ptr(valid)))
        return offsets, out[: total.value], valid.astype(bool)

    def _rows_device(self, fn, ids, orientations, predecessors):
        ids, orient = self._queries(ids, orientations)
        out = EdgeRows()
        check(fn(self._h, self._ws, _ptr(ids), _ptr(orient), ids.size, int(bool(predecessors)), C.byref(out)))
        return out

    def _one_row(self, rows):
        offsets, out, valid = rows
        return [(int(x) >> 1, int(x) & 1) for x in out] if valid[0] else None

    def edges_csr(self, node_ids, orientations, predecessors=False):
        """GBZ::successors / predecessors (src/gbz.rs:327-353) for a batch of (node id, orientation): (offsets[u64, n + 1], edges[u64], valid[bool]);
        an edge is 2 * id + orientation; valid[k] is False, with an empty row, where the reference returns None.  `orientations`: an array, or
        one value for all."""
        return self._rows_csr(self._L.gbwt_hip_edges, node_ids, orientations, predecessors)

    def edges_device(self, node_ids, orientations, predecessors=False):
        """The same rows left in HBM: an EdgeRows struct (d_offsets u64[n + 1], d_edges u64[total], d_valid u8[n]), valid until the next edges /
        links request on this workspace.  rows_to_host() copies them out."""
        return self._rows_device(self._L.gbwt_hip_edges_device, node_ids, orientations, predecessors)

    def rows_to_host(self, rows):
        """(offsets, edges, valid) of an edges_device() / links_device() result (through torch views of the workspace's memory)."""
        import torch
        from . import dist as D
        device = torch.device("cuda", self._device)
        offsets = D.device_view(rows.d_offsets, (rows.n + 1) * 8, torch.uint8, device).cpu().numpy().view(np.uint64)
        edges = D.device_view(rows.d_edges, rows.total * 8, torch.uint8, device).cpu().numpy().view(np.uint64) if rows.total else np.zeros(0, np.uint64)
        valid = D.device_view(rows.d_valid, rows.n, torch.uint8, device).cpu().numpy() if rows.n else np.zeros(0, np.uint8)
        return offsets.copy(), edges.copy(), valid.astype(bool)

    def successors(self, node_id, orientation):
        """GBZ::successors(node_id, orientation): a list of (id, orientation), or None (src/gbz.rs:327-335)."""
        return self._one_row(self.edges_csr([node_id], [orientation], False))

    def predecessors(self, node_id, orientation):
        """GBZ::predecessors(node_id, orientation): a list of (id, orientation), or None (src/gbz.rs:345-353)."""
        return self._one_row(self.edges_csr([node_id], [orientation], True))

    # ---- search -------------------------------------------------------------------------------
    def find(self, nodes):
        nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
        out = np.zeros(nodes.size, dtype=STATE_DTYPE)
        valid = np.zeros(nodes.size, dtype=np.uint8)
        check(self._L.gbwt_hip_find(self._h, self._ws, _ptr(nodes), nodes.size, _ptr(out), _ptr(valid)))
        return out, valid.astype(bool)

    def extend(self, states, nodes):
        states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
        nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
        assert states.size == nodes.size
        out = np.zeros(nodes.size, dtype=STATE_DTYPE)
        valid = np.zeros(nodes.size, dtype=np.uint8)
        check(self._L.gbwt_hip_extend(self._h, self._ws, _ptr(states), _ptr(nodes), nodes.size, _ptr(out), _ptr(valid)))
        return out, valid.astype(bool)

    def bd_find(self, nodes):
        nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
        out = np.zeros(nodes.size, dtype=BD_DTYPE)
        valid = np.zeros(nodes.size, dtype=np.uint8)
        check(self._L.gbwt_hip_bd_find(self._h, self._ws, _ptr(nodes), nodes.size, _ptr(out), _ptr(valid)))
        return out, valid.astype(bool)

    def _bd_extend(self, fn, states, nodes):
        states = np.ascontiguousarray(states, dtype=BD_DTYPE)
        nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
        assert states.size == nodes.size
        out = np.zeros(nodes.size, dtype=BD_DTYPE)
        valid = np.zeros(nodes.size, dtype=np.uint8)
        check(fn(self._h, self._ws, _ptr(states), _ptr(nodes), nodes.size, _ptr(out), _ptr(valid)))
        return out, valid.astype(bool)

    def extend_forward(self, states, nodes):
        return self._bd_extend(self._L.gbwt_hip_extend_forward, states, nodes)

    def extend_backward(self, states, nodes):
        return self._bd_extend(self._L.gbwt_hip_extend_backward, states, nodes)

    def follow(self, states, backward=False):
        """GBZ::follow_forward / follow_backward (src/gbz.rs:519-544) for an array of bidirectional states:
        (offsets[n + 1], extensions, valid); valid[i] is False where the reference returns no iterator."""
        st = np.ascontiguousarray(states, dtype=BD_DTYPE)
        offsets = np.zeros(st.size + 1, dtype=np.uint64)
        valid = np.zeros(st.size, dtype=np.uint8)
        total = C.c_uint64(0)
        check(self._L.gbwt_hip_follow(self._h, self._ws, _ptr(st), st.size, int(backward), _ptr(offsets), None, 0, C.byref(total), _ptr(valid)))
        out = np.zeros(max(total.value, 1), dtype=BD_DTYPE)
        check(self._L.gbwt_hip_follow(self._h, self._ws, _ptr(st), st.size, int(backward), _ptr(offsets), _ptr(out), out.size, C.byref(total), _ptr(valid)))
        return offsets, out[:total.value], valid.astype(bool)

    @staticmethod
    def _results(n, dtype, out):
        """Result arrays of a host-pointer query call: fresh ones, or the caller's `out` = (states, valid uint8) of the right shape -- a caller
        that asks again and again keeps its arrays: the device-to-host copy into pages that have been touched takes half the time of the copy
        into fresh ones (profiles/r06_download_probe.txt)."""
        if out is None:
            return np.zeros(n, dtype=dtype), np.zeros(n, dtype=np.uint8)
        states, valid = out
        assert states.dtype == dtype and states.shape == (n,) and states.flags.c_contiguous and valid.dtype == np.uint8 and valid.shape == (n,) and valid.flags.c_contiguous
        return states, valid

    def search(self, queries, out=None):
        """find(q[0]) + extend over q[1:] for every row of the (n, len) query matrix (src/bin/benchmark.rs:155-169).  `out`: see _results."""
        q = np.ascontiguousarray(queries, dtype=np.uint64)
        assert q.ndim == 2
        out, valid = self._results(q.shape[0], STATE_DTYPE, out)
        check(self._L.gbwt_hip_search(self._h, self._ws, _ptr(q), q.shape[0], q.shape[1], _ptr(out), _ptr(valid)))
        return out, valid.astype(bool)

    def search_device(self, d_queries, n, length):
        """gbwt_hip_search_device: `d_queries` = device pointer (int) to an n x length u64 matrix in HBM; the final states stay in the
        workspace: a _lib.States struct (d_states, d_valid, n).  states_to_host() copies them out."""
        out = _lib.States()
        check(self._L.gbwt_hip_search_device(self._h, self._ws, C.c_void_p(int(d_queries)), n, length, C.byref(out)))
        return out

    def states_to_host(self, states, bidirectional=False):
        """(states, valid) of a search_device() / bd_search_device() result as host arrays (through torch views of the workspace's memory)."""
        import torch
        from . import dist as D
        dtype = BD_DTYPE if bidirectional else STATE_DTYPE
        device = torch.device("cuda", self._device)
        raw = D.device_view(states.d_states, states.n * dtype.itemsize, torch.uint8, device).cpu().numpy()
        valid = D.device_view(states.d_valid, states.n, torch.uint8, device).cpu().numpy()
        return raw.view(dtype).copy(), valid.astype(bool)

    def bd_search_device(self, d_queries, n, length, first):
        out = _lib.States()
        check(self._L.gbwt_hip_bd_search_device(self._h, self._ws, C.c_void_p(int(d_queries)), n, length, first, C.byref(out)))
        return out

    def bd_search(self, queries, first, out=None):
        """bd_find(q[first]) then alternating extend_forward / extend_backward over every row of the query matrix.  `out`: see _results."""
        q = np.ascontiguousarray(queries, dtype=np.uint64)
        assert q.ndim == 2
        out, valid = self._results(q.shape[0], BD_DTYPE, out)
        check(self._L.gbwt_hip_bd_search(self._h, self._ws, _ptr(q), q.shape[0], q.shape[1], first, _ptr(out), _ptr(valid)))
        return out, valid.astype(bool)


    # ---- locate: the sequences behind a search state (any handle) -----------------------------------
    @staticmethod
    def _structured(values, dtype, what):
        """A one-dimensional contiguous array of `dtype` (STATE_DTYPE / POS_DTYPE) from such an array, an (n, fields) unsigned integer matrix
        or a list of tuples."""
        if isinstance(values, np.ndarray) and values.dtype == dtype:
            a = values
        else:
            try:
                raw = np.asarray(values)
            except Exception as e:  # noqa: BLE001
                raise TypeError(f"{what} must be an array of {dtype} or an (n, {len(dtype.names)}) integer matrix") from e
            if raw.dtype.names is not None:
                raise TypeError(f"{what} have dtype {raw.dtype}, expected {dtype}")
            if raw.size == 0:
                raw = np.zeros((0, len(dtype.names)), dtype=np.uint64)
            if raw.dtype.kind not in "ui":
                raise TypeError(f"{what} must hold integers, not {raw.dtype}")
            if raw.ndim != 2 or raw.shape[1] != len(dtype.names):
                raise ValueError(f"{what} must have shape (n, {len(dtype.names)}), not {raw.shape}")
            if raw.dtype.kind == "i" and raw.size and raw.min() < 0:
                raise ValueError(f"{what} must not be negative")
            a = np.ascontiguousarray(raw, dtype=np.uint64).view(dtype).reshape(-1)
        if a.ndim != 1:
            raise ValueError(f"{what} must be one-dimensional, not of shape {a.shape}")
        return np.ascontiguousarray(a)

    def locate_csr(self, states, unique=False):
        """The sequences behind a batch of search states (node, start, end): (offsets[u64, n + 1], ids[u64], valid[bool]).  Row k holds the
        id of the sequence that owns offset start, start + 1, ... of the node's record in that order (unique=False), or the same ids ascending
        without duplicates (unique=True, the C++ GBWT's locate(SearchState)).  valid[k] is False, with an empty row, where the node has no
        record, start >= end or end exceeds the record's length.  The first call on a handle builds its locate index."""
        st = self._structured(states, STATE_DTYPE, "states")
        offsets = np.zeros(st.size + 1, dtype=np.uint64)
        valid = np.zeros(st.size, dtype=np.uint8)
        total = C.c_uint64(0)
        check(self._L.gbwt_hip_locate(self._h, self._ws, _ptr(st), st.size, int(bool(unique)), _ptr(offsets), None, 0, C.byref(total), _ptr(valid)))
        ids = np.zeros(max(1, total.value), dtype=np.uint64)
        check(self._L.gbwt_hip_locate(self._h, self._ws, _ptr(st), st.size, int(bool(unique)), _ptr(offsets), _ptr(ids), ids.size, C.byref(total), _ptr(valid)))
        return offsets, ids[: total.value], valid.astype(bool)

    def locate(self, state, unique=True):
        """The sequence ids of one state (node, start, end) as a numpy uint64 array, or None for a state that is no range of a record."""
        state = tuple(int(x) for x in state)
        if len(state) != 3:
            raise ValueError("a state is (node, start, end)")
        offsets, ids, valid = self.locate_csr(np.array([state], dtype=STATE_DTYPE), unique)
        return ids.copy() if valid[0] else None

    def locate_device(self, states, unique=False):
        """The rows of locate_csr left in HBM: a _lib.Located struct (d_offsets u64[n + 1], d_ids u64[total], d_valid u8[n]), valid until the next
        locate request on this workspace; edges / links requests leave it alone.  located_to_host() copies it out."""
        st = self._structured(states, STATE_DTYPE, "states")
        out = Located()
        check(self._L.gbwt_hip_locate_device(self._h, self._ws, _ptr(st), st.size, int(bool(unique)), C.byref(out)))
        return out

    def locate_states_device(self, states_struct, unique=False):
        """locate_device for states that are in HBM already: the _lib.States of search_device() (failed searches, d_valid == 0, are invalid
        rows).  Search -> locate never leaves the device."""
        if not isinstance(states_struct, _lib.States):
            raise TypeError("locate_states_device takes the _lib.States struct of search_device()")
        out = Located()
        check(self._L.gbwt_hip_locate_states_device(self._h, self._ws, states_struct.d_states, states_struct.d_valid, states_struct.n, int(bool(unique)), C.byref(out)))
        return out

    def located_to_host(self, rows):
        """(offsets, ids, valid) of a locate_device() / locate_states_device() result (through torch views of the workspace's memory)."""
        import torch
        from . import dist as D
        device = torch.device("cuda", self._device)
        offsets = D.device_view(rows.d_offsets, (rows.n + 1) * 8, torch.uint8, device).cpu().numpy().view(np.uint64)
        ids = D.device_view(rows.d_ids, rows.total * 8, torch.uint8, device).cpu().numpy().view(np.uint64) if rows.total else np.zeros(0, np.uint64)
        valid = D.device_view(rows.d_valid, rows.n, torch.uint8, device).cpu().numpy() if rows.n else np.zeros(0, np.uint8)
        return offsets.copy(), ids.copy(), valid.astype(bool)

    def locate_positions(self, positions):
        """The C++ GBWT's locate(node, i) for a batch of positions (node, offset): (ids[u64], valid[bool]); valid[k] is False, with id 0, where
        the node has no record (the endmarker included) or the offset is past the record."""
        pos = self._structured(positions, POS_DTYPE, "positions")
        ids = np.zeros(pos.size, dtype=np.uint64)
        valid = np.zeros(pos.size, dtype=np.uint8)
        check(self._L.gbwt_hip_locate_positions(self._h, self._ws, _ptr(pos), pos.size, _ptr(ids), _ptr(valid)))
        return ids, valid.astype(bool)

    def last_locate_ms(self):
        """(walk_ms, sort_ms) of the last locate request for states on this workspace (HIP events); sort_ms is 0 unless it was unique."""
        walk, sort = C.c_float(0), C.c_float(0)
        check(self._L.gbwt_hip_last_locate_ms(self._ws, C.byref(walk), C.byref(sort)))
        return walk.value, sort.value

    def locate_count_steps(self, states):
        """(LF steps, located positions) of the plain rows of `states`: the locate kernel launched once more with a counter (a measurement)."""
        st = self._structured(states, STATE_DTYPE, "states")
        steps, positions = C.c_uint64(0), C.c_uint64(0)
        check(self._L.gbwt_hip_locate_count_steps(self._h, self._ws, _ptr(st), st.size, C.byref(steps), C.byref(positions)))
        return steps.value, positions.value

    def locate_index_info(self):
        """The locate index of the handle (gbwt_hip_locate_index_info) as a dict; all zeros before the first locate call."""
        info = LocateInfo()
        check(self._L.gbwt_hip_locate_index_info(self._h, C.byref(info)))
        return _as_dict(info, skip_reserved=True)


class GBZ(GBWT):
    """gbz::GBZ for the hot path: GBZ::path / paths (src/gbz.rs:446-466)."""

    @staticmethod
    def _gfa_options(max_node, translate):
        """gbwt_hip_gfa_options of the two keywords, or None for the call without options.  max_node alone chops where a segment is longer
        (translate = AUTO); translate alone chops nothing."""
        if max_node is None and translate is None:
            return None
        if translate is None:
            translate = _lib.GFA_TRANSLATE_AUTO
        return _lib.GfaOptions(int(max_node or 0), int(translate))

    @classmethod
    def from_gfa(cls, path, device=0, flags=_lib.OPEN_ALL, max_node=None, translate=None):
        """The GBZ of a GFA file, parsed and constructed on the device (gbwt_hip_build_from_gfa): gbunzip's inverse.  What is accepted:
        include/gbwt_hip.h, "construction from GFA".  max_node (segments longer than that many bases are chopped into nodes; gfa2gbwt's
        default is 1024) and translate (GFA_TRANSLATE_NEVER | _AUTO | _ALWAYS) build a node-to-segment translation, for segment names that
        are no node ids (gbwt_hip_build_from_gfa_opts); both None is the call without options."""
        h = C.c_void_p()
        opts = cls._gfa_options(max_node, translate)
        check(_lib.lib().gbwt_hip_build_from_gfa_opts(os.fsencode(path), _ref_or_null(opts), device, flags, C.byref(h)))
        return cls(h, device=device)

    @classmethod
    def from_gfa_text(cls, data, device=0, flags=_lib.OPEN_ALL, max_node=None, translate=None):
        """The same for a GFA text in memory: bytes, a bytearray, or a str (encoded as UTF-8)."""
        if isinstance(data, str):
            data = data.encode()
        text = np.frombuffer(bytes(data), dtype=np.uint8)
        h = C.c_void_p()
        opts = cls._gfa_options(max_node, translate)
        check(_lib.lib().gbwt_hip_build_from_gfa_text_opts(_ptr(text), text.size, _ref_or_null(opts), device, flags, C.byref(h)))
        return cls(h, device=device)

    def last_gfa_translation_info(self):
        """The translation behind a handle made from GFA (gbwt_hip_last_gfa_translation_info): a dict; all zeros for every other handle."""
        g = _lib.GfaTranslationInfo()
        check(self._L.gbwt_hip_last_gfa_translation_info(self._h, C.byref(g)))
        return _as_dict(g, skip_reserved=True)

    def last_gfa_info(self):
        """The parse behind a handle made from GFA (gbwt_hip_last_gfa_info): a dict; all zeros for every other handle."""
        g = GfaInfo()
        check(self._L.gbwt_hip_last_gfa_info(self._h, C.byref(g)))
        return _as_dict(g)

    def paths(self):
        return self.sequences() // 2

    def path(self, path_id, orientation=FORWARD):
        """GBZ::path(path_id, orientation): list of (node_id, orientation), or None (src/gbz.rs:461-466)."""
        seq = self.sequence(encode_path(path_id, orientation))
        return None if seq is None else [decode_node(x) for x in seq]

    def path_lines(self, path_ids, mode):
        """gbunzip's P-lines (mode 0), W-lines (mode 1) or P-lines with PanSN names (mode 2) for the given paths, as bytes
        (src/bin/gbunzip.rs:438-550)."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        total = C.c_uint64(0)
        check(self._L.gbwt_hip_path_lines(self._h, self._ws, _ptr(ids), ids.size, mode, None, 0, C.byref(total)))
        buf = C.create_string_buffer(max(1, total.value))
        check(self._L.gbwt_hip_path_lines(self._h, self._ws, _ptr(ids), ids.size, mode, buf, total.value, C.byref(total)))
        return buf.raw[: total.value]

    def path_lines_array(self, path_ids, mode, out=None):
        """The same lines as a numpy uint8 array -- into `out` when it is large enough (a reused buffer has its pages already) --
        without the zero-filled ctypes buffer and the second copy `path_lines` pays for a bytes object."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        total = C.c_uint64(0)
        check(self._L.gbwt_hip_path_lines(self._h, self._ws, _ptr(ids), ids.size, mode, None, 0, C.byref(total)))
        if out is None or out.size < total.value:
            out = np.empty(max(1, total.value), dtype=np.uint8)
        check(self._L.gbwt_hip_path_lines(self._h, self._ws, _ptr(ids), ids.size, mode, out.ctypes.data, out.size, C.byref(total)))
        return out[: total.value]

    def last_lines_ms(self):
        """(walk kernel ms, everything behind the walk ms) of the last path_lines / path_lines_device request (HIP events)."""
        walk, fmt = C.c_float(0), C.c_float(0)
        check(self._L.gbwt_hip_last_lines_ms(self._ws, C.byref(walk), C.byref(fmt)))
        return walk.value, fmt.value

    def write_gfa(self, path, path_mode=PATHS_DEFAULT):
        """The file `gbunzip -t 1 --paths MODE` writes for this GBZ (src/bin/gbunzip.rs:205-226; PathMode 63-76)."""
        check(self._L.gbwt_hip_write_gfa_mode(self._h, self._ws, os.fsencode(path), path_mode))

    def paths_csr(self, path_ids, orientation=FORWARD):
        """GBZ::path(id, orientation) for every id, as CSR of GBWT-encoded nodes (support::encode_path, src/support.rs:229-231)."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        return self.sequences_csr(2 * ids + np.uint64(1 if orientation else 0))

    def segment_paths(self, seq_ids):
        """GBZ::segment_path (src/gbz.rs:477-489) for a batch of SEQUENCE ids (2 * path + orientation): (offsets[n + 1], tokens) with token =
        (segment id << 1) | orientation -- the (Segment, Orientation) pairs SegmentPathIter yields, up to the place where it stops for a path
        that is not a concatenation of whole segments.  GbwtHipError(BAD_ARGUMENT) without a node-to-segment translation (the reference: None)."""
        ids = np.ascontiguousarray(seq_ids, dtype=np.uint64)
        offsets = np.zeros(ids.size + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        check(self._L.gbwt_hip_segment_paths(self._h, self._ws, _ptr(ids), ids.size, _ptr(offsets), None, 0, C.byref(total)))
        tokens = np.zeros(max(total.value, 1), dtype=np.uint64)
        check(self._L.gbwt_hip_segment_paths(self._h, self._ws, _ptr(ids), ids.size, _ptr(offsets), _ptr(tokens), tokens.size, C.byref(total)))
        return offsets, tokens[:total.value]

    def segment_path(self, path_id, orientation=FORWARD):
        """[(segment id, orientation), ...] of one path (GBZ::segment_path(path_id, orientation))."""
        _, tokens = self.segment_paths([2 * path_id + (1 if orientation else 0)])
        return [(int(t) >> 1, int(t) & 1) for t in tokens]

    @staticmethod
    def _endmarker(endmarker):
        if endmarker is None:
            return -1
        if isinstance(endmarker, (bytes, bytearray)):
            if len(endmarker) != 1:
                raise ValueError("endmarker must be one byte")
            return endmarker[0]
        e = int(endmarker)
        if not 0 <= e <= 255:
            raise ValueError("endmarker must be None or a byte value 0..255")
        return e

    def path_sequences(self, path_ids, orientation=FORWARD, endmarker=None, out=None):
        """The bases of every path (gbz-extract's extract_sequence, src/bin/gbz-extract.rs:173-189): labels joined along GBZ::path(id,
        orientation), reverse-oriented ones reverse-complemented, `endmarker` (None or a byte value) behind every row.  Returns (offsets[n + 1],
        bases): bytes, or a view of `out` -- a writable C-contiguous uint8 array, used when it is large enough.  A path id without such a
        sequence gives an empty row without endmarker."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        em, rev = self._endmarker(endmarker), 1 if orientation else 0
        if out is not None:
            if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 1 or not out.flags.c_contiguous or not out.flags.writeable:
                raise TypeError("out must be a writable C-contiguous 1-d numpy uint8 array")
        offsets = np.zeros(ids.size + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        check(self._L.gbwt_hip_path_sequences(self._h, self._ws, _ptr(ids), ids.size, rev, em, None, _ptr(offsets), 0, C.byref(total)))
        if out is not None and out.size >= total.value:
            check(self._L.gbwt_hip_path_sequences(self._h, self._ws, _ptr(ids), ids.size, rev, em, _ptr(out), None, out.size, C.byref(total)))
            return offsets, out[: total.value]
        buf = np.empty(max(1, total.value), dtype=np.uint8)
        check(self._L.gbwt_hip_path_sequences(self._h, self._ws, _ptr(ids), ids.size, rev, em, buf.ctypes.data, None, buf.size, C.byref(total)))
        return offsets, buf[: total.value].tobytes()

    def path_sequences_device(self, path_ids, orientation=FORWARD, endmarker=None):
        """The same bases left in HBM: a Lines struct (d_text, d_line_offsets[n + 1], total, n), valid until the next request for bases on
        this workspace."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        out = Lines()
        check(self._L.gbwt_hip_path_sequences_device(self._h, self._ws, _ptr(ids), ids.size, 1 if orientation else 0, self._endmarker(endmarker), C.byref(out)))
        return out

    def last_sequences_ms(self):
        """(walk ms, sizing ms, bases kernel ms) of the last path_sequences / path_sequences_device request (HIP events)."""
        walk, sizes, bases = C.c_float(0), C.c_float(0), C.c_float(0)
        check(self._L.gbwt_hip_last_sequences_ms(self._ws, C.byref(walk), C.byref(sizes), C.byref(bases)))
        return walk.value, sizes.value, bases.value

    def node_sequence(self, node_id):
        """GBZ::sequence(node_id) (src/gbz.rs:292-298): the label as bytes, or None for a node that does not exist."""
        length, found = C.c_uint64(0), C.c_uint8(0)
        check(self._L.gbwt_hip_node_sequence(self._h, int(node_id), None, 0, C.byref(length), C.byref(found)))
        if not found.value:
            return None
        buf = C.create_string_buffer(max(1, length.value))
        check(self._L.gbwt_hip_node_sequence(self._h, int(node_id), buf, length.value, C.byref(length), C.byref(found)))
        return buf.raw[: length.value]

    @staticmethod
    def _contig(contig):
        if contig is None or isinstance(contig, bytes):
            return contig
        if isinstance(contig, str):
            return contig.encode()
        raise TypeError("contig must be None, str or bytes")

    def remove_contig(self, name, algorithm=None, flags=_lib.OPEN_ALL):
        """The GBZ without the paths select_paths(contig=name) gives: the whole component in which a path with that contig name starts."""
        return self.remove_paths(self.select_paths(contig=name), algorithm=algorithm, flags=flags)

    def select_paths(self, contig=None):
        """select_paths of gbz-extract (src/bin/gbz-extract.rs:196-264): every path id for contig=None; otherwise the ascending ids of every path
        whose first node lies in a weakly connected component in which a path with that contig name starts.  GbwtHipError(BAD_ARGUMENT) with the
        reference's messages: no contig names, an unknown contig, a contig no path carries."""
        name = self._contig(contig)
        total = C.c_uint64(0)
        check(self._L.gbwt_hip_select_paths(self._h, self._ws, name, None, 0, C.byref(total)))
        out = np.zeros(max(1, total.value), dtype=np.uint64)
        check(self._L.gbwt_hip_select_paths(self._h, self._ws, name, _ptr(out), out.size, C.byref(total)))
        return out[: total.value]

    def write_sequences(self, path, path_ids=None, endmarker=0, contig=None):
        """The files `gbz-extract -o path` writes (src/bin/gbz-extract.rs:266-294): the forward bases of the paths (None = all) with an
        endmarker behind each (None: none), and `path`.names.  contig=NAME is `gbz-extract -c NAME`: the paths select_paths(NAME) gives."""
        if contig is not None:
            if path_ids is not None:
                raise ValueError("contig and path_ids exclude each other")
            check(self._L.gbwt_hip_write_sequences_contig(self._h, self._ws, os.fsencode(path), self._contig(contig), self._endmarker(endmarker)))
            return
        ids = None if path_ids is None else np.ascontiguousarray(path_ids, dtype=np.uint64)
        n = 0 if ids is None else ids.size
        if ids is not None and ids.size == 0:
            ids = np.zeros(1, dtype=np.uint64)             # (an empty list is not NULL = all paths)
        ptr = None if ids is None else ids.ctypes.data
        check(self._L.gbwt_hip_write_sequences(self._h, self._ws, os.fsencode(path), ptr, n, self._endmarker(endmarker)))

    def text_length(self, path_ids):
        """The length of the text gbz-extract's `sequences` mode writes for these paths (the bases of every path and one endmarker each): the
        expected_len of its `tag-array` mode (src/bin/gbz-extract.rs:408-411)."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        expected = C.c_uint64(0)
        check(self._L.gbwt_hip_tags(self._h, self._ws, _ptr(ids), ids.size, None, 0, None, C.byref(expected), None))
        return expected.value

    def tag_array(self, path_ids, sa, return_runs=False):
        """gbz-extract's tag array (src/bin/gbz-extract.rs:346-371, 408-470) for the text of these paths: TAG[i] = the graph position of
        text position sa[i] -- ((node id << 11) | (orientation << 10)) + the offset inside the node, 0 for an endmarker -- as a numpy uint64
        array [, the number of runs].  GbwtHipError(INVALID_DATA) for a value >= text_length(path_ids)."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        sa = np.ascontiguousarray(sa, dtype=np.uint64)
        if sa.ndim != 1:
            raise ValueError("sa must be one-dimensional")
        tags = np.zeros(sa.size, dtype=np.uint64)
        runs = C.c_uint64(0)
        if sa.size:
            check(self._L.gbwt_hip_tags(self._h, self._ws, _ptr(ids), ids.size, _ptr(sa), sa.size, _ptr(tags), None, C.byref(runs)))
        else:
            self.text_length(ids)                          # (the checks of the request, nothing to look up)
        return (tags, runs.value) if return_runs else tags

    def tags_device(self, path_ids, d_sa, count, d_tags):
        """gbwt_hip_tags_device: `d_sa` and `d_tags` are device pointers (int) to `count` uint64 values in HBM -- any slice of a suffix array --
        and stay there; returns the runs of these entries."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        runs = C.c_uint64(0)
        check(self._L.gbwt_hip_tags_device(self._h, self._ws, _ptr(ids), ids.size, C.c_void_p(int(d_sa)), count, C.c_void_p(int(d_tags)), C.byref(runs)))
        return runs.value

    def write_tag_array(self, base, sa_skip=1):
        """`gbz-extract -m tag-array -o base` (src/bin/gbz-extract.rs:408-482): reads `base`.names and `base`.sa (sa_skip leading values
        skipped), writes `base`.tags; returns the reference's "Tag array runs"."""
        runs = C.c_uint64(0)
        check(self._L.gbwt_hip_write_tag_array(self._h, self._ws, os.fsencode(base), sa_skip, C.byref(runs)))
        return runs.value

    def last_tags_ms(self):
        """(walk ms, plan ms, gather kernel ms) of the last request for tags (HIP events; the plan's while it is reused)."""
        walk, plan, gather = C.c_float(0), C.c_float(0), C.c_float(0)
        check(self._L.gbwt_hip_last_tags_ms(self._ws, C.byref(walk), C.byref(plan), C.byref(gather)))
        return walk.value, plan.value, gather.value

    def suffix_array(self, path_ids, endmarker=0, return_bwt=False):
        """The suffix array of the text path_sequences(path_ids, FORWARD, endmarker) returns (gbwt_hip_path_suffix_array), built on the device
        from the bases there: a numpy uint64 array, or with return_bwt (sa, bwt uint8, runs of the bwt); the byte in front of suffix 0 is the
        endmarker (0 without one)."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        em = self._endmarker(endmarker)
        total, runs = C.c_uint64(0), C.c_uint64(0)
        check(self._L.gbwt_hip_path_suffix_array(self._h, self._ws, _ptr(ids), ids.size, em, None, None, 0, C.byref(total), C.byref(runs)))
        sa = np.zeros(total.value, dtype=np.uint64)
        bwt = np.zeros(total.value, dtype=np.uint8) if return_bwt else None
        if total.value:
            check(self._L.gbwt_hip_path_suffix_array(self._h, self._ws, _ptr(ids), ids.size, em, _ptr(sa), _ptr(bwt), sa.size, C.byref(total), C.byref(runs)))
        return (sa, bwt, runs.value) if return_bwt else sa

    def suffix_array_device(self, path_ids, endmarker=0):
        """The same left in HBM: a SuffixArray struct (d_sa u64[total], d_bwt u8[total], total, bwt_runs), valid until the next suffix array
        request on this workspace; d_sa is an argument for tags_device as it is."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        out = SuffixArray()
        check(self._L.gbwt_hip_path_suffix_array_device(self._h, self._ws, _ptr(ids), ids.size, self._endmarker(endmarker), C.byref(out)))
        return out

    def write_suffix_array(self, base):
        """What stands between `gbz-extract -o base` and `gbz-extract -m tag-array -o base`: reads `base`.names (and the endmarker at the end
        of `base`), writes `base`.sa and `base`.bwt as write_tag_array(base) and the reference read them; returns the runs of the BWT."""
        runs = C.c_uint64(0)
        check(self._L.gbwt_hip_write_suffix_array(self._h, self._ws, os.fsencode(base), C.byref(runs)))
        return runs.value

    def fm_index(self, path_ids, endmarker=0, count_only=False, keep_text=False):
        """The FM-index of the text path_sequences(path_ids, FORWARD, endmarker) returns (gbwt_hip_path_fm_index): a PathFMIndex, built on the
        device from the text and suffix array of suffix_array_device(path_ids, endmarker).  endmarker: a byte value, not None.  keep_text:
        the object keeps the text as well (PathFMIndex.keep_text), for alignments."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        if endmarker is None:
            raise ValueError("an FM-index of paths needs an endmarker: the tags of the text count one behind every path")
        handle = C.c_void_p()
        check(self._L.gbwt_hip_path_fm_index(self._h, self._ws, _ptr(ids), ids.size, self._endmarker(endmarker), _lib.FM_COUNT_ONLY if count_only else 0, C.byref(handle)))
        fm = PathFMIndex(handle, self._device, owner=self)
        if keep_text:
            fm.keep_text()
        return fm

    def last_suffix_array_info(self):
        """The last suffix array built on this workspace (gbwt_hip_last_suffix_array_info): a dict -- n, rounds, active (the active set behind
        the first keys and behind every round), round_ms, peak_scratch_bytes, planned_scratch_bytes, text_ms, pack_ms, rank_ms, output_ms."""
        return _suffix_info(self._ws)

    # ---- the graph: segments, links, GFA lines -----------------------------------------------------
    def has_translation(self):
        """GBZ::has_translation (src/gbz.rs:362-364)."""
        return bool(self._stats.has_translation)

    def node_to_segments(self, node_ids):
        """GBZ::node_to_segment (src/gbz.rs:370-376) for a batch: (segment ids[u64], valid[bool])."""
        ids = np.ascontiguousarray(node_ids, dtype=np.uint64)
        out = np.zeros(ids.size, dtype=np.uint64)
        valid = np.zeros(ids.size, dtype=np.uint8)
        check(self._L.gbwt_hip_node_segments(self._h, _ptr(ids), ids.size, _ptr(out), _ptr(valid)))
        return out, valid.astype(bool)

    def node_to_segment(self, node_id):
        """The id of the segment that holds the node, or None without a translation or without the node."""
        out, valid = self.node_to_segments([node_id])
        return int(out[0]) if valid[0] else None

    def segment_iter(self):
        """GBZ::segment_iter (src/gbz.rs:381-390): the ids of the segments whose first node exists (numpy uint64), or None without a translation."""
        if not self.has_translation():
            return None
        total = C.c_uint64(0)
        check(self._L.gbwt_hip_segments(self._h, None, 0, C.byref(total)))
        out = np.zeros(max(1, total.value), dtype=np.uint64)
        check(self._L.gbwt_hip_segments(self._h, _ptr(out), out.size, C.byref(total)))
        return out[: total.value]

    def links_csr(self, segment_ids, orientations, predecessors=False):
        """GBZ::segment_successors / segment_predecessors (src/gbz.rs:402-440) for a batch of (segment id, orientation): (offsets, links, valid);
        a link is 2 * segment id + orientation."""
        return self._rows_csr(self._L.gbwt_hip_links, segment_ids, orientations, predecessors)

    def links_device(self, segment_ids, orientations, predecessors=False):
        """The same rows left in HBM (an EdgeRows struct; rows_to_host() copies them out)."""
        return self._rows_device(self._L.gbwt_hip_links_device, segment_ids, orientations, predecessors)

    def segment_successors(self, segment_id, orientation):
        """A list of (segment id, orientation), or None (GBZ::segment_successors, src/gbz.rs:402-415)."""
        return self._one_row(self.links_csr([segment_id], [orientation], False))

    def segment_predecessors(self, segment_id, orientation):
        """A list of (segment id, orientation), or None (GBZ::segment_predecessors, src/gbz.rs:427-440)."""
        return self._one_row(self.links_csr([segment_id], [orientation], True))

    def graph_lines(self):
        """The H-line, the S-lines and the L-lines gbunzip writes for this graph (src/bin/gbunzip.rs:193-332), formatted on the device, as bytes."""
        total = C.c_uint64(0)
        check(self._L.gbwt_hip_graph_lines(self._h, self._ws, None, 0, C.byref(total)))
        buf = np.empty(max(1, total.value), dtype=np.uint8)
        check(self._L.gbwt_hip_graph_lines(self._h, self._ws, buf.ctypes.data, buf.size, C.byref(total)))
        return buf[: total.value].tobytes()

    def graph_lines_device(self):
        """The same text left in HBM: a GraphText struct (d_text; header_bytes, segment_bytes, link_bytes; segments, links = the line counts).
        Every call formats again; the sizes are kept from the first one."""
        out = GraphText()
        check(self._L.gbwt_hip_graph_lines_device(self._h, self._ws, C.byref(out)))
        return out

    def last_graph_ms(self):
        """(sizing ms, S-lines ms, L-lines ms) of the last graph lines request (HIP events; sizing is 0 where the kept sizes were used)."""
        sizes, segments, links = C.c_float(0), C.c_float(0), C.c_float(0)
        check(self._L.gbwt_hip_last_graph_ms(self._ws, C.byref(sizes), C.byref(segments), C.byref(links)))
        return sizes.value, segments.value, links.value

    # ---- reference positions ---------------------------------------------------------------------
    def reference_sample_names(self, also_generic):
        """GBZ::reference_sample_names (src/gbz.rs:183-196): the names of the GBWT tag `reference_samples` (split at ' ') and, with
        also_generic, `_gbwt_ref`, those that the metadata's sample dictionary holds.  Nothing without metadata."""
        total = C.c_uint64(0)
        check(self._L.gbwt_hip_reference_sample_names(self._h, int(bool(also_generic)), None, 0, C.byref(total)))
        buf = C.create_string_buffer(max(1, total.value))
        check(self._L.gbwt_hip_reference_sample_names(self._h, int(bool(also_generic)), buf, total.value, C.byref(total)))
        return [name.decode() for name in buf.raw[: total.value].split(b"\n")[:-1]]

    def reference_paths(self, also_generic=True):
        """The ids (uint64, ascending) of the paths whose sample is a reference sample (src/gbz.rs:609-629).  GbwtHipError(BAD_ARGUMENT)
        without metadata."""
        count = C.c_uint64(0)
        check(self._L.gbwt_hip_reference_paths(self._h, int(bool(also_generic)), None, 0, C.byref(count)))
        out = np.zeros(max(1, count.value), dtype=np.uint64)
        check(self._L.gbwt_hip_reference_paths(self._h, int(bool(also_generic)), _ptr(out), out.size, C.byref(count)))
        return out[: count.value]

    def path_positions_csr(self, path_ids, interval):
        """gbwt_hip_path_positions: (paths[REFPATH_DTYPE, n], positions[REFPOS_DTYPE, total]); the positions of row k are
        positions[paths[k].first : paths[k].first + paths[k].count]."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        if ids.ndim != 1:
            raise ValueError("path_ids must be one-dimensional")
        paths = np.zeros(ids.size, dtype=REFPATH_DTYPE)
        total = C.c_uint64(0)
        check(self._L.gbwt_hip_path_positions(self._h, self._ws, _ptr(ids), ids.size, int(interval), _ptr(paths), None, 0, C.byref(total)))
        positions = np.zeros(max(1, total.value), dtype=REFPOS_DTYPE)
        check(self._L.gbwt_hip_path_positions(self._h, self._ws, _ptr(ids), ids.size, int(interval), None, _ptr(positions), positions.size, C.byref(total)))
        return paths, positions[: total.value]

    @staticmethod
    def _reference_rows(paths, positions):
        rows = []
        for p in paths:
            part = positions[int(p["first"]):int(p["first"] + p["count"])]
            rows.append((int(p["path_id"]), int(p["len"]), part["offset"].copy(), np.stack([part["node"], part["pos_offset"]], axis=1)))
        return rows

    def path_positions(self, path_ids, interval):
        """GBZ::reference_positions' rule (src/gbz.rs:630-648) for any forward path ids, in the order given, a duplicate as a row of its own:
        a list of (id, len, offsets uint64[k], positions uint64[k, 2] = (node, offset) of bwt::Pos).  About every `interval` bases the base
        offset of a node start and the GBWT position of that visit; len = the bases of the path."""
        return self._reference_rows(*self.path_positions_csr(path_ids, interval))

    def path_positions_device(self, path_ids, interval):
        """The same left in HBM: (d_paths, d_positions, total) -- device pointers (int) to n gbwt_hip_reference_path and `total`
        gbwt_hip_reference_position (24 bytes), valid until the next request for positions on this workspace."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        d_paths, d_positions, total = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        check(self._L.gbwt_hip_path_positions_device(self._h, self._ws, _ptr(ids), ids.size, int(interval), C.byref(d_paths), C.byref(d_positions), C.byref(total)))
        return d_paths.value or 0, d_positions.value or 0, total.value

    def reference_positions(self, interval):
        """GBZ::reference_positions(interval) (src/gbz.rs:600-657): for every reference path, ascending, (id, len, offsets uint64[k],
        positions uint64[k, 2]).  GbwtHipError: BAD_ARGUMENT without metadata, UNSUPPORTED for a bare GBWT."""
        n, total = C.c_uint64(0), C.c_uint64(0)
        check(self._L.gbwt_hip_reference_positions(self._h, self._ws, int(interval), None, 0, C.byref(n), None, 0, C.byref(total)))
        paths = np.zeros(max(1, n.value), dtype=REFPATH_DTYPE)
        positions = np.zeros(max(1, total.value), dtype=REFPOS_DTYPE)
        check(self._L.gbwt_hip_reference_positions(self._h, self._ws, int(interval), _ptr(paths), paths.size, C.byref(n), _ptr(positions), positions.size, C.byref(total)))
        return self._reference_rows(paths[: n.value], positions[: total.value])

    def last_positions_ms(self):
        """(walk ms, selection ms, offsets walk ms) of the last request for positions (HIP events)."""
        walk, select, offsets = C.c_float(0), C.c_float(0), C.c_float(0)
        check(self._L.gbwt_hip_last_positions_ms(self._ws, C.byref(walk), C.byref(select), C.byref(offsets)))
        return walk.value, select.value, offsets.value

    def last_positions_rounds(self):
        """(pointer-doubling rounds that marked something, launches behind the extraction) of the last request for positions."""
        rounds, launches = C.c_uint32(0), C.c_uint32(0)
        check(self._L.gbwt_hip_last_positions_rounds(self._ws, C.byref(rounds), C.byref(launches)))
        return rounds.value, launches.value

    def path_lines_device(self, path_ids, mode):
        """The same lines left in HBM: a Lines struct (device pointers to the text and to the n + 1 line offsets)."""
        ids = np.ascontiguousarray(path_ids, dtype=np.uint64)
        out = Lines()
        check(self._L.gbwt_hip_path_lines_device(self._h, self._ws, _ptr(ids), ids.size, mode, C.byref(out)))
        return out


__all__ = ["GBWT", "GBZ", "GbwtHipError", "Components", "EdgeRows", "GraphText", "Lines", "Paths", "FORWARD", "REVERSE", "PATHS_DEFAULT", "PATHS_PAN_SN", "PATHS_REF_ONLY", "POS_DTYPE", "STATE_DTYPE", "BD_DTYPE", "REFPATH_DTYPE", "REFPOS_DTYPE", "encode_node",
           "decode_node", "flip_node", "encode_path", "device_count", "device_memory", "parse_file", "Pos", "State", "BdState"]
