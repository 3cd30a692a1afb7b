/*
 * gbwt_hip.h -- C ABI of libgbwt_hip.so: the MI355X (gfx950) drop-in for the GBWT LF-step hot path
 * of jltsiren/gbwt-rs (crate `gbz` 0.5.1).
 *
 * The reference has no FFI of its own (no `extern`, no build.rs); every entry point below names the
 * Rust interface it replaces (file:line into the reference repository) and mirrors its semantics in
 * batched form.  Plain pointers and sizes only; no torch / HIP types in any signature (streams and
 * device buffers are passed as `void *`).  INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions:
 *   - every function returns a gbwt_hip_status; 0 = success.  "Not found" is a value
 *     (Option::None <-> valid[i] = 0), never an error.
 *   - a handle is immutable after open and safe for concurrent read-only calls from several host
 *     threads as long as each thread uses its own gbwt_hip_workspace (the reference shares &GBZ across
 *     rayon workers, src/bin/gbunzip.rs:421-434).
 *   - malformed *files* -> GBWT_HIP_INVALID_DATA (io::ErrorKind::InvalidData in the reference);
 *     where the reference asserts/panics (non-bidirectional index in bd_* calls) -> GBWT_HIP_BAD_ARGUMENT.
 *   - there is NO CPU fallback: without a usable HIP device every compute call fails with
 *     GBWT_HIP_NO_DEVICE / GBWT_HIP_DEVICE_ERROR.
 *
 * Widths.  The reference is usize (u64) everywhere (bwt::Pos, src/bwt.rs:63-69); this ABI carries u64 in every struct, but the
 * device side computes in u32: node ids, record indices, offsets inside a record and rank-block indices.  An index outside that
 * range is refused AT OPEN with GBWT_HIP_UNSUPPORTED (never truncated, never a wrong answer later):
 *     alphabet_size > 2^32                          (node ids; SURVEY 8b allows u32 node ids iff alphabet_size <= 2^32)
 *     2^30 records or more                          (bits 30-31 of a record word carry flags)
 *     a record with 2^32 or more positions          (Record::len: offsets inside a record are u32; counted by the device pass at open)
 *     (size >> 6) + records >= 2^32 - 16            (rank-block indices)
 * Sequence lengths are u32 as well: an index in which one sequence has 2^32 - 16 or more nodes opens without sequence lengths and
 * samples (extractions then take the pool-output kernel).  Record byte streams and CSR outputs are 64-bit throughout (an index
 * whose rank blocks exceed 4 GiB is walked with 64-bit block addresses).  Query inputs are u64 and compared as such: a node or
 * offset that does not fit u32 cannot exist in an index that was opened, and yields "not found" (valid = 0).
 */
#ifndef GBWT_HIP_H
#define GBWT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    GBWT_HIP_OK = 0,
    GBWT_HIP_INVALID_DATA = 1, /* io::ErrorKind::InvalidData: bad tag/version/flags, length mismatch, ... */
    GBWT_HIP_IO_ERROR = 2,     /* file cannot be opened / read */
    GBWT_HIP_BAD_ARGUMENT = 3, /* id out of range, index not bidirectional, null pointer, ... */
    GBWT_HIP_NO_DEVICE = 4,    /* no HIP device available */
    GBWT_HIP_DEVICE_ERROR = 5, /* a HIP runtime call failed */
    GBWT_HIP_CAPACITY = 6,     /* caller-provided output capacity too small (total is still reported) */
    GBWT_HIP_UNSUPPORTED = 7   /* e.g. alphabet_size > 2^32 (u32 node ids on device) */
} gbwt_hip_status;

/* bwt::Pos, src/bwt.rs:63-69 */
typedef struct { uint64_t node, offset; } gbwt_hip_pos;
/* gbwt::SearchState, src/gbwt.rs:455-460 (range = start..end) */
typedef struct { uint64_t node, start, end; } gbwt_hip_state;
/* gbwt::BidirectionalState, src/gbwt.rs:485-490 */
typedef struct { gbwt_hip_state forward, reverse; } gbwt_hip_bd_state;

/* GBWT statistics: len/sequences/alphabet_size/alphabet_offset/is_bidirectional/has_metadata,
 * src/gbwt.rs:108-182; records = BWT::len (src/bwt.rs:105-107). */
typedef struct {
    uint64_t size;            /* GBWT::len */
    uint64_t sequences;       /* GBWT::sequences */
    uint64_t alphabet_size;   /* GBWT::alphabet_size */
    uint64_t alphabet_offset; /* GBWT::alphabet_offset */
    uint64_t records;         /* BWT::len */
    uint64_t data_bytes;      /* length of the record byte stream */
    uint64_t paths;           /* metadata path names (0 if none) */
    uint32_t bidirectional;   /* GBWT::is_bidirectional */
    uint32_t has_metadata;    /* GBWT::has_metadata */
    uint32_t is_gbz;          /* file was a GBZ container (graph + translation available) */
    uint32_t has_translation; /* Graph::has_translation, src/graph.rs:158-160 */
    uint64_t max_record_len;  /* largest Record::len over all records (device pass at open) */
    uint64_t max_outdegree;   /* largest Record::outdegree */
} gbwt_hip_stats;

typedef struct gbwt_hip_index gbwt_hip_index;         /* opaque: host + device copies of one index */
typedef struct gbwt_hip_workspace gbwt_hip_workspace; /* opaque: per-caller device scratch + stream */

/* Message for the last failing call on this thread. */
const char *gbwt_hip_last_error(void);
/* Number of visible HIP devices (0 on a CPU-only box; never fails). */
int gbwt_hip_device_count(void);

/* ---- load --------------------------------------------------------------------------------------
 * Replaces simple_sds::serialize::load_from::<GBWT | GBZ> (src/gbwt.rs:402-438, src/gbz.rs:674-717).
 * Detects GBWT vs GBZ by the header tag, rejects what the reference rejects (src/headers.rs:101-115,
 * 229-231; src/bwt.rs:179-181; src/gbz.rs:684-692) and uploads the record stream, the dense record
 * start array (decoded from the Elias-Fano index) and the decompressed endmarker (src/gbwt.rs:413-414)
 * to `device`.
 * THE FILE STAYS MAPPED while the handle is open (files of 4 MB or more): the host's own copy of the record bytes and starts -- read by the
 * S / L lines of gbwt_hip_write_gfa* and by a node-to-segment translation, by nothing else -- is made from the mapping when it is first
 * needed, not by the open (3.5 GB and 0.4 s of a 1.0 s open for an HPRC-sized GBZ).  Replace such a file by rename, never truncate or
 * rewrite it in place under an open handle.  GBWT_HIP_LAZY_HOST_RECORDS=0 in the environment: the copy is made by the open, as until round 5. */
gbwt_hip_status gbwt_hip_open_file(const char *path, int device, gbwt_hip_index **out);

/* Host-only parse + validation of a .gbwt/.gbz (no device needed): what load_from would accept. */
gbwt_hip_status gbwt_hip_parse_file(const char *path, gbwt_hip_stats *out);

/* Replaces constructing a GBWT from an in-memory BWT: the thin Rust shim passes the raw record stream
 * it already owns -- base pointer from BWT::compressed_record(0) (src/bwt.rs:134-143), record starts
 * recovered per record -- plus the header fields (src/gbwt.rs:108-174).  `starts` has n_records
 * entries; record i spans [starts[i], starts[i+1]) and the last one ends at data_len
 * (BWT::record_bytes, src/bwt.rs:116-121).  Inputs are borrowed only for the call. */
gbwt_hip_status gbwt_hip_open_records(const uint8_t *data, uint64_t data_len, const uint64_t *starts,
                                      uint64_t n_records, uint64_t alphabet_offset, uint64_t alphabet_size,
                                      uint64_t n_sequences, uint64_t size, int bidirectional, int device,
                                      gbwt_hip_index **out);
/* The same with a statement of what the handle is FOR (round 5): an index is replicated per GPU and most of what a handle holds in HBM
 * is built for one group of entry points only, so a caller that names its group pays for that group:
 *   GBWT_HIP_OPEN_EXTRACT  gbwt_hip_extract*, path sums / hashes / copies: walk descriptors (64 + 128 B per record), rank blocks and packed
 *                          two-step half-blocks (16 + 32 B per 64 positions of an outdegree-2 record), walk tables, sequence lengths + samples
 *   GBWT_HIP_OPEN_SEARCH   start / forward / backward / find / extend / bd_* / follow / search: raw descriptors (64 B per record), rank
 *                          blocks (16 B per 64 positions), LF tables of the records with outdegree > 2 (16 B per position)
 *   GBWT_HIP_OPEN_GFA      gbwt_hip_path_lines*, gbwt_hip_write_gfa* (implies EXTRACT): label lengths, translation and line header tables
 * A handle opened WITHOUT SEARCH whose walks never leave the descriptors and rank blocks (no record of outdegree > 2, no edge that failed
 * a check at open) also gives back, once it is open, what only the open itself, the search kernels and the non-default walk modes read: the
 * raw descriptors, the one-step walk descriptors and the plain rank blocks (128 B per record + 16 B per 64 positions: config 4 at its
 * stated size 65 -> 36 GB, the headline index 3.3 -> 2.2 GB); the catch-up steps of the walk then read the two-step descriptors and the
 * packed half-blocks, and the pool-output walk modes of gbwt_hip_workspace_tune return GBWT_HIP_UNSUPPORTED.
 * Record bytes, record starts and the endmarker are always there.  An entry point outside the handle's groups returns
 * GBWT_HIP_BAD_ARGUMENT.  gbwt_hip_open_file / gbwt_hip_open_records = GBWT_HIP_OPEN_ALL.  Config 3's index (1.1 M sites x 5 008
 * haplotypes): 11.4 GB opened for everything, 3.6 GB for SEARCH; gbwt_hip_memory_usage reports what a handle holds. */
enum { GBWT_HIP_OPEN_EXTRACT = 1, GBWT_HIP_OPEN_SEARCH = 2, GBWT_HIP_OPEN_GFA = 4, GBWT_HIP_OPEN_ALL = 7 };
gbwt_hip_status gbwt_hip_open_file_flags(const char *path, int device, uint32_t flags, gbwt_hip_index **out);
gbwt_hip_status gbwt_hip_open_records_flags(const uint8_t *data, uint64_t data_len, const uint64_t *starts,
                                            uint64_t n_records, uint64_t alphabet_offset, uint64_t alphabet_size,
                                            uint64_t n_sequences, uint64_t size, int bidirectional, int device, uint32_t flags,
                                            gbwt_hip_index **out);
void gbwt_hip_close(gbwt_hip_index *index);
gbwt_hip_status gbwt_hip_get_stats(const gbwt_hip_index *index, gbwt_hip_stats *out);

/* What a handle and a workspace hold (bytes).  index_device_bytes: every array of the handle in HBM -- the record bytes, starts,
 * descriptors, rank blocks, tables, samples, GFA tables; the full-width two-step blocks are counted once they have been built (on first
 * need).  An index is replicated per GPU, so this is also the cost of one more rank.  index_host_bytes: the host image (record
 * bytes, starts, names, node labels).  workspace_device_bytes (0 for ws == NULL): all scratch of the workspace, of which rows_bytes are
 * the extracted rows (the CSR node ids) and text_bytes the formatted GFA lines and the bases of paths; the plan and the staging of
 * gbwt_hip_tags* are workspace scratch.  The node labels of a GBZ are in
 * index_device_bytes once the first request for bases has made them, the weakly connected components once the first call for them has. */
typedef struct {
    uint64_t index_device_bytes, index_host_bytes;
    uint64_t workspace_device_bytes, rows_bytes, text_bytes;
    uint64_t rows_chunks;   /* physical chunks the rows are mapped from (virtual-memory API, GBWT_HIP_VMM); 0 = one hipMalloc */
} gbwt_hip_memory;
gbwt_hip_status gbwt_hip_memory_usage(const gbwt_hip_index *index, const gbwt_hip_workspace *ws, gbwt_hip_memory *out);

/* Where the time of gbwt_hip_open_* went (host clock, milliseconds; the one-shot flow of gbunzip, src/bin/gbunzip.rs:24-59, pays all
 * of it once per file): parse_ms = reading and validating the file (0 for gbwt_hip_open_records), upload_ms = host-to-device copies
 * and the per-record passes (descriptors, rank blocks, tables, endmarker), sample_ms = sequence lengths + sequence samples,
 * total_ms = the whole call.  samples = sequence samples built; checkpoint_sampling = 1 when they came from checkpoint sampling
 * (no sequence walked from end to end), with its number of launches, walkers, and hops that ended at the length cap (orphans).
 * line_sizes_ms (inside upload_ms; handles opened for GFA lines) = the walk that sizes the GFA line of every path once, at open -- token
 * bytes per 4 096 positions and summed label lengths, i.e. the W-line's end coordinate (src/bin/gbunzip.rs:532-540) -- so that no
 * gbwt_hip_path_lines* request sizes a line: 0 where the handle has no such table (no GFA group, a node-to-segment translation, no
 * sequence samples). */
typedef struct {
    double parse_ms, upload_ms, sample_ms, total_ms;
    uint64_t samples, checkpoint_walkers, checkpoint_orphans;
    uint32_t checkpoint_sampling, checkpoint_rounds;
    double line_sizes_ms;
} gbwt_hip_open_times;
gbwt_hip_status gbwt_hip_get_open_times(const gbwt_hip_index *index, gbwt_hip_open_times *out);

/* Workspaces own a HIP stream and reusable device scratch (path pool, CSR outputs). */
gbwt_hip_status gbwt_hip_workspace_create(const gbwt_hip_index *index, gbwt_hip_workspace **out);
void gbwt_hip_workspace_destroy(gbwt_hip_workspace *ws);
/* Tuning of the extraction kernel for this workspace (results never depend on it):
 *   walk_mode      0 = one lane per sequence, two LF steps per iteration on the two-step rank blocks built at open (default),
 *                  1 = lane-serial scan from the start of every record (the reference's access pattern),
 *                  2 = wave-cooperative decode of long records (all 64 lanes scan one record's runs),
 *                  3 = one lane per sequence, one LF step per iteration on the plain rank blocks
 *   paths_per_wave lanes of each wavefront that own a sequence, 1..64; 0 = automatic (default): at least 32 owners per
 *                  wave -- the walk is latency-bound, not throughput-bound, and every lane runs the same instructions
 *   small_record   mode 2 only: records of at most this many bytes are decoded by their own lane (default 16)
 * Environment overrides read at workspace creation: GBWT_HIP_WALK_MODE, GBWT_HIP_PATHS_PER_WAVE, GBWT_HIP_SMALL_RECORD. */
gbwt_hip_status gbwt_hip_workspace_tune(gbwt_hip_workspace *ws, uint32_t walk_mode, uint32_t paths_per_wave, uint32_t small_record);
/* The hipStream_t the workspace launches on (for event timing by the caller). */
void *gbwt_hip_workspace_stream(gbwt_hip_workspace *ws);

/* ---- path extraction ---------------------------------------------------------------------------
 * gbwt_hip_extract: GBWT::sequence(id).collect::<Vec<_>>() for every id (src/gbwt.rs:253-261,
 * SequenceIter::next 557-568).  CSR output: out_offsets[n+1], nodes of sequence k at
 * out_nodes[out_offsets[k] .. out_offsets[k+1]).  id >= sequences (the reference returns no iterator) and
 * an empty sequence both give a zero-length row: "not found" never fails the batch, and the caller tells
 * the two apart by id < sequences.  `*total` always receives the number of nodes (= LF steps); with
 * out_nodes == NULL it is a size query; if capacity < total the call returns GBWT_HIP_CAPACITY.  Host
 * buffers.  The sequences are walked ONCE per request: the rows stay in the workspace, and the call that
 * repeats the ids of the previous gbwt_hip_extract / gbwt_hip_extract_device on it (the fill call after a
 * size query) only copies them out.  gbwt_hip_follow and gbwt_hip_path_lines do the same. */
gbwt_hip_status gbwt_hip_extract(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *seq_ids,
                                 uint64_t n, uint64_t *out_offsets, uint32_t *out_nodes, uint64_t capacity,
                                 uint64_t *total);

/* Device-resident form: results stay in HBM inside the workspace (valid until the next call on it).
 * d_offsets: uint64_t[n+1], d_nodes: uint32_t[total] (device pointers).  This is what bench.py times. */
typedef struct { const uint64_t *d_offsets; const uint32_t *d_nodes; uint64_t total; uint64_t n; } gbwt_hip_paths;
gbwt_hip_status gbwt_hip_extract_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws,
                                        const uint64_t *seq_ids, uint64_t n, gbwt_hip_paths *out);

/* One part of every row (round 4; SURVEY 8e's partition, cut the other way): the rows of gbwt_hip_extract_device are cut where their
 * walkers start anyway -- at the sequence samples the index made at open -- into `parts` stretches of (nearly) equal numbers of samples, and
 * this call walks and returns stretch `part` of every row only: row k of the result is nodes [from_k, to_k) of GBWT::sequence(seq_ids[k]),
 * and the stretches part = 0 .. parts - 1 of a row, back to back, are the row (rows with fewer samples than parts leave some stretches
 * empty; an index opened without samples gives the whole row as the LAST part).  This is how N GPUs share one batch: every rank walks
 * EVERY path over ITS N-th of the way -- it reads an N-th of the index and keeps whole waves on every record -- instead of every N-th
 * path over the whole way (measured on one GPU, an eighth of the headline batch: 0.53-0.60 ms per pass against 0.88 ms;
 * profiles/r04_shard_probe.txt); gbwt_hip_gather_rows(..., GBWT_HIP_GATHER_PARTS, ...) puts the rows together.  parts = 1 is
 * gbwt_hip_extract_device. */
gbwt_hip_status gbwt_hip_extract_part_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *seq_ids, uint64_t n,
                                             uint32_t part, uint32_t parts, gbwt_hip_paths *out);

/* Copies the last device-resident extraction of `ws` to host buffers: out_offsets[n + 1] and/or out_nodes[total]
 * (either may be NULL; capacity < total -> GBWT_HIP_CAPACITY).  With gbwt_hip_extract_device this is "extract once,
 * size the buffer from gbwt_hip_paths.total, copy". */
gbwt_hip_status gbwt_hip_copy_result(const gbwt_hip_index *index, gbwt_hip_workspace *ws, uint64_t *out_offsets,
                                     uint32_t *out_nodes, uint64_t capacity);

/* GBZ::path(path_id, orientation) (src/gbz.rs:461-466, PathIter 1053-1059): sequence id =
 * 2*path_id + orientation (support::encode_path, src/support.rs:229-231); output nodes stay GBWT-encoded
 * (node_id = v / 2, orientation = v & 1: support::decode_node, src/support.rs:180-182). */
gbwt_hip_status gbwt_hip_extract_paths(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *path_ids,
                                       uint64_t n, int reverse, uint64_t *out_offsets, uint32_t *out_nodes,
                                       uint64_t capacity, uint64_t *total);

/* ---- navigation --------------------------------------------------------------------------------
 * GBWT::start (src/gbwt.rs:213-219) and GBWT::forward (222-229) for n independent inputs. */
gbwt_hip_status gbwt_hip_start(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *seq_ids, uint64_t n,
                               gbwt_hip_pos *out, uint8_t *valid);
gbwt_hip_status gbwt_hip_forward(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const gbwt_hip_pos *in, uint64_t n,
                                 gbwt_hip_pos *out, uint8_t *valid);
/* GBWT::backward (src/gbwt.rs:236-250): Record::predecessor_at (src/bwt.rs:502-540) on the record of the flipped node,
 * then Record::offset_to (558-584) in the predecessor's record.  The reference asserts a bidirectional index; here a
 * unidirectional one returns GBWT_HIP_BAD_ARGUMENT. */
gbwt_hip_status gbwt_hip_backward(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const gbwt_hip_pos *in, uint64_t n,
                                  gbwt_hip_pos *out, uint8_t *valid);

/* ---- search ------------------------------------------------------------------------------------
 * GBWT::find (src/gbwt.rs:269-281), GBWT::extend (292-304). */
gbwt_hip_status gbwt_hip_find(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *nodes, uint64_t n,
                              gbwt_hip_state *out, uint8_t *valid);
gbwt_hip_status gbwt_hip_extend(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const gbwt_hip_state *states,
                                const uint64_t *nodes, uint64_t n, gbwt_hip_state *out, uint8_t *valid);
/* GBWT::bd_find (311-324), extend_forward (339-347), extend_backward (362-367).  The reference asserts a
 * bidirectional index; here a unidirectional one returns GBWT_HIP_BAD_ARGUMENT. */
gbwt_hip_status gbwt_hip_bd_find(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *nodes, uint64_t n,
                                 gbwt_hip_bd_state *out, uint8_t *valid);
gbwt_hip_status gbwt_hip_extend_forward(const gbwt_hip_index *index, gbwt_hip_workspace *ws,
                                        const gbwt_hip_bd_state *states, const uint64_t *nodes, uint64_t n,
                                        gbwt_hip_bd_state *out, uint8_t *valid);
gbwt_hip_status gbwt_hip_extend_backward(const gbwt_hip_index *index, gbwt_hip_workspace *ws,
                                         const gbwt_hip_bd_state *states, const uint64_t *nodes, uint64_t n,
                                         gbwt_hip_bd_state *out, uint8_t *valid);
/* GBZ::follow_forward / follow_backward + StateIter (src/gbz.rs:519-544, 1211-1251): every non-empty extension of each
 * state by one node, listed in the order of the edge list (EdgeIter, src/gbz.rs:819-855).  CSR output: the extensions
 * of state i are out_states[out_offsets[i] .. out_offsets[i+1]); valid[i] = 0 where the reference returns no iterator
 * (GBZ::successors: the node does not exist).  `*total` always receives the number of extensions; out_states == NULL
 * is a size query (out_offsets and valid are still filled); capacity < total -> GBWT_HIP_CAPACITY. */
gbwt_hip_status gbwt_hip_follow(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const gbwt_hip_bd_state *states, uint64_t n,
                                int backward, uint64_t *out_offsets, gbwt_hip_bd_state *out_states, uint64_t capacity,
                                uint64_t *total, uint8_t *valid);
/* Whole query in one launch, the shape of src/bin/benchmark.rs:155-169: for query q (row q of the
 * n x len matrix `queries`), find(q[0]) then extend by q[1..]; out/valid describe the final state
 * (valid = 0 as soon as any step returns None). */
gbwt_hip_status gbwt_hip_search(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *queries,
                                uint64_t n, uint64_t len, gbwt_hip_state *out, uint8_t *valid);

/* Bidirectional form of the same: bd_find(q[first]), then alternately extend_forward over q[first+1..] and
 * extend_backward over q[first-1..0] until both ends of the row are consumed (the usage pattern of
 * GBWT::bd_find / extend_forward / extend_backward, src/gbwt.rs:311-367). */
gbwt_hip_status gbwt_hip_bd_search(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *queries,
                                   uint64_t n, uint64_t len, uint64_t first, gbwt_hip_bd_state *out, uint8_t *valid);

/* Device-resident forms (round 5): the queries are in HBM already (`d_queries`: n x len u64, a device pointer of the caller, read on the
 * workspace stream), the final states stay in HBM inside the workspace (valid until the next query call on it): d_states[n], d_valid[n].
 * What a pipeline that produces its queries on the GPU calls, and what separates the kernel from PCIe: a million 10-node queries are
 * 80 MB in and 25 MB out around a 0.5 ms kernel: a host-pointer call is bound by PCIe (3 ms), whichever way the copies are staged
 * (GBWT_HIP_QUERY_PIPELINE, profiles/r05_query_call_sweep.txt). */
typedef struct { const gbwt_hip_state *d_states; const uint8_t *d_valid; uint64_t n; } gbwt_hip_states;
typedef struct { const gbwt_hip_bd_state *d_states; const uint8_t *d_valid; uint64_t n; } gbwt_hip_bd_states;
gbwt_hip_status gbwt_hip_search_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *d_queries, uint64_t n, uint64_t len,
                                       gbwt_hip_states *out);
gbwt_hip_status gbwt_hip_bd_search_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *d_queries, uint64_t n, uint64_t len,
                                          uint64_t first, gbwt_hip_bd_states *out);

/* ---- GFA text (GBZ handles with metadata) ------------------------------------------------------------
 * gbwt_hip_path_lines: the lines gbunzip writes for the given paths, in the order given, byte for byte:
 * mode 0 = P-lines named by the contig (write_p_line / path_to_p_line, src/bin/gbunzip.rs:438-485), mode 1 = W-lines
 * (path_to_w_line, src/bin/gbunzip.rs:495-550), mode 2 = P-lines with PanSN names sample#phase#contig (path_to_pan_sn,
 * src/bin/gbunzip.rs:487-491; Metadata::pan_sn_path, src/gbwt.rs:709-713).  The forward sequences are walked and the node tokens
 * formatted on the device; the host only contributes the name fields.  `*total` receives the number of bytes;
 * out == NULL is a size query; capacity < total -> GBWT_HIP_CAPACITY.  Graphs with a node-to-segment
 * translation print segment names (GBZ::segment_path / SegmentPathIter, src/gbz.rs:477-486, 1098-1169). */
gbwt_hip_status gbwt_hip_path_lines(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n,
                                    int mode, char *out, uint64_t capacity, uint64_t *total);
/* Device-resident form: the text stays in HBM inside the workspace (valid until the next GFA call on it); line k is
 * d_text[d_line_offsets[k] .. d_line_offsets[k + 1]).  This is what a multi-GPU extraction hands to the RCCL gather
 * (gbwt_rs_amd/dist.py) and what gbwt_hip_path_lines copies out. */
typedef struct { const char *d_text; const uint64_t *d_line_offsets; uint64_t total; uint64_t n; } gbwt_hip_lines;
gbwt_hip_status gbwt_hip_path_lines_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *path_ids,
                                           uint64_t n, int mode, gbwt_hip_lines *out);
/* GBZ::segment_path(path, orientation) for a batch of SEQUENCE ids (2 * path + orientation; src/gbz.rs:477-489, SegmentPathIter 1098-1169):
 * a CSR of tokens, token = (segment id << 1) | orientation (0 forward, 1 reverse) -- the (Segment, Orientation) pairs the iterator yields, the
 * segment as its index in the translation (GBZ::segment_iter order; names and sequences belong to the host's Graph).  A path that is not a
 * concatenation of whole segments yields the tokens up to the place where the reference's iterator stops.  GBWT_HIP_BAD_ARGUMENT for a graph
 * without a node-to-segment translation (the reference returns None) and for a handle that was not opened for GFA lines.  out_offsets has n + 1
 * entries; out_tokens NULL = size query (*total = tokens of all rows; the rows are walked again by the fill call). */
gbwt_hip_status gbwt_hip_segment_paths(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *seq_ids, uint64_t n, uint64_t *out_offsets,
                                       uint64_t *out_tokens, uint64_t capacity, uint64_t *total);
/* gbwt_hip_write_gfa: the whole file `gbunzip -t 1` writes (write_gfa_impl, src/bin/gbunzip.rs:205-226, default
 * path mode): H, S and L lines from the host copy of the graph, then P-lines and W-lines in ascending path id. */
gbwt_hip_status gbwt_hip_write_gfa(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const char *path);
/* The same with gbunzip's `--paths MODE` (PathMode, src/bin/gbunzip.rs:63-76; dispatch 212-222): default = P-lines of the paths of
 * the generic sample `_gbwt_ref`, then W-lines of all others; pan-sn = every path as a P-line with its PanSN name (write_pan_sn,
 * 371-393); ref-only = the P-lines of the default mode and nothing else. */
enum { GBWT_HIP_PATHS_DEFAULT = 0, GBWT_HIP_PATHS_PAN_SN = 1, GBWT_HIP_PATHS_REF_ONLY = 2 };
gbwt_hip_status gbwt_hip_write_gfa_mode(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const char *path, int path_mode);

/* ---- bases of paths (GBZ handles opened with GBWT_HIP_OPEN_EXTRACT) --------------------------------------------------------------
 * gbz-extract's `sequences` mode (src/bin/gbz-extract.rs:173-194, 266-294).  The bases of a path are GBZ::sequence(node) joined along
 * GBZ::path(path_id, orientation) (src/gbz.rs:292-305, 461-466), the label of a reverse-oriented node reverse-complemented
 * (support::reverse_complement, src/support.rs:87-110: A, C, G, T in either case to the upper-case complement, every other byte to N).
 * The node labels reach HBM on the first such request on a handle (one upload whichever thread asks first; counted in
 * gbwt_hip_memory_usage's index_device_bytes from then on); an open never makes them.  A handle that is not a GBZ, or was not opened for
 * extraction, gives GBWT_HIP_BAD_ARGUMENT; so does an endmarker outside -1 .. 255.
 *
 * gbwt_hip_path_sequences_device: extract_sequence (src/bin/gbz-extract.rs:173-189) for every path id, in the order given, orientation
 * Reverse where `reverse` != 0; `endmarker` = -1: none, 0 .. 255: that byte behind every row (gbz-extract's --endmarker-value, default 0).
 * Row k = d_text[d_line_offsets[k] .. d_line_offsets[k + 1]) (device pointers, valid until the next request for bases on `ws`).  A path id
 * whose sequence 2 id + orientation does not exist gives an empty row without endmarker (as gbwt_hip_extract_paths, whose rows these are). */
gbwt_hip_status gbwt_hip_path_sequences_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int reverse,
                                               int endmarker, gbwt_hip_lines *out);
/* The same copied to host buffers: out_offsets[n + 1] (may be NULL), out[total]; out == NULL is a size query, capacity < total ->
 * GBWT_HIP_CAPACITY.  `*total` always receives the bytes.  The fill call that repeats the request of a size query does not walk again. */
gbwt_hip_status gbwt_hip_path_sequences(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int reverse, int endmarker,
                                        char *out, uint64_t *out_offsets, uint64_t capacity, uint64_t *total);
/* GBZ::sequence / sequence_len (src/gbz.rs:292-305) from the host image: *found = 0 for a node that does not exist (GBZ::has_node,
 * src/gbz.rs:286-289; not an error), else *len = the label's bytes and, unless out == NULL (size query), the label in out[0 .. len);
 * capacity < len -> GBWT_HIP_CAPACITY.  GBWT_HIP_BAD_ARGUMENT for a bare GBWT. */
gbwt_hip_status gbwt_hip_node_sequence(const gbwt_hip_index *index, uint64_t node_id, char *out, uint64_t capacity, uint64_t *len, uint8_t *found);
/* gbz-extract -o path (extract_sequences, src/bin/gbz-extract.rs:266-294), byte for byte: the forward bases of the given paths (NULL = all,
 * ascending), each followed by `endmarker` (-1: none), into `path`, and for every path the line path_name_as_line writes (:191-194)
 * "path_id \t sample \t contig \t phase \t fragment \t bases \n" into `path`.names (names fall back to the number, src/gbwt.rs:755-761,
 * 803-809).  Batches bounded by bytes (GBWT_HIP_SEQ_BATCH_MIB, read at each call; default 1024) go through two device buffers while a writer
 * thread moves the previous one to the file.  GBWT_HIP_BAD_ARGUMENT without metadata or path names, and for a path id out of range. */
gbwt_hip_status gbwt_hip_write_sequences(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const char *path, const uint64_t *path_ids, uint64_t n, int endmarker);
/* Device time of the last request for bases on `ws` (HIP events): *walk_ms = the walk of its extraction, *sizes_ms = sizing and placing its rows
 * up to the host's one wait, *bases_ms = the chunk plan and the bases kernel. */
gbwt_hip_status gbwt_hip_last_sequences_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *sizes_ms, float *bases_ms);

/* ---- tags of a suffix array (GBZ handles opened with GBWT_HIP_OPEN_EXTRACT) ------------------------------------------------------------
 * gbz-extract's `tag-array` mode (src/bin/gbz-extract.rs:296-482).  The TEXT of paths p_0 .. p_{n-1}, in the order given, is what
 * gbwt_hip_write_sequences writes for them: the forward bases of p_0, one endmarker, the bases of p_1, one endmarker, ...; row k starts at
 * off_k = sum of (len_j + 1) over j < k, and expected_len = off_{n-1} + len_{n-1} + 1 (0 for n = 0).  The TAG of text position t
 * (extract_path / encode_start, :346-371) is 0 for an endmarker, and otherwise ((v << 11) | (o << 10)) + w for the base that lies w bases --
 * in reading direction, also on a reverse node -- behind the first base of the step (node id v, orientation o: 1 = reverse) of GBZ::path(p_k,
 * Forward) it falls into.  Nodes are nodes, never segments.  The sum is a plain 64-bit addition: like the reference (its FIXME) nothing guards
 * labels longer than 1 024 bases, whose w carries into the orientation bit and the node id.  TAG[i] = tag(SA[i]): what the reference's two
 * sorts compute when the values they read are a permutation of 0 .. expected_len - 1; for other input the reference's result is unspecified,
 * ours is this gather.  A value >= expected_len is GBWT_HIP_INVALID_DATA and is never read through.  RUNS: the number of i with
 * TAG[i] != TAG[i - 1], the first entry of a request counting as one (the reference's "Tag array runs").
 *
 * The map from text offsets to walk positions (the PLAN: 12 bytes per node of the paths + 1 per 8 text positions) is made by the first
 * request for a list of path ids and stays on the workspace, counted in workspace_device_bytes, while the list stays the same.  A plan, or
 * the staging of a request, that does not fit in free device memory is GBWT_HIP_CAPACITY with a message that says what was needed.
 * Preconditions as for gbwt_hip_path_sequences*: GBWT_HIP_BAD_ARGUMENT for a bare GBWT, a handle without GBWT_HIP_OPEN_EXTRACT, and a path id
 * without a sequence 2 id.
 *
 * gbwt_hip_tags_device: d_tags[i] = tag(d_sa[i]) for i < count, both in HBM; `count` is any number of entries (a slice of a suffix array
 * is fine); *runs (may be NULL) for these entries.  After GBWT_HIP_INVALID_DATA the contents of d_tags are unspecified (nothing was written
 * for the offending entries). */
gbwt_hip_status gbwt_hip_tags_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, const uint64_t *d_sa, uint64_t count,
                                     uint64_t *d_tags, uint64_t *runs);
/* The same with host pointers.  *expected_len (may be NULL) always receives the text length; sa == NULL and tags == NULL is the size query
 * that returns it.  After an error `tags` is untouched. */
gbwt_hip_status gbwt_hip_tags(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, const uint64_t *sa, uint64_t count,
                              uint64_t *tags, uint64_t *expected_len, uint64_t *runs);
/* gbz-extract -m tag-array -o base (extract_tag_array, :408-482): reads `base`.names (one line per path: first tab field = path id, last =
 * bases; the metadata is not needed) and `base`.sa (little-endian u64: sa_skip values are skipped -- the reference's default is 1 -- then
 * expected_len are read), writes `base`.tags: exactly 8 * expected_len bytes, the tags as little-endian u64 without a header.  The suffix array
 * streams through two pairs of device buffers in batches bounded by bytes (GBWT_HIP_TAG_BATCH_MIB, read at each call; default 256) while a
 * writer thread moves the previous batch of tags to the file.  GBWT_HIP_INVALID_DATA: an empty .names ("No path names found"), a line that
 * does not parse, a path whose walked bases differ from its line ("Invalid length for path P: expected L, got M"), a value out of range;
 * GBWT_HIP_IO_ERROR: a file that cannot be opened, a .sa shorter than sa_skip + expected_len values.  No .tags file stays behind a failure. */
gbwt_hip_status gbwt_hip_write_tag_array(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const char *base_path, uint64_t sa_skip, uint64_t *runs);
/* Device time of the last request for tags on `ws` (HIP events): *walk_ms = the walk of the plan's extraction, *plan_ms = the rest of the plan
 * (both those of the request that made the plan, while it is reused), *gather_ms = the gather kernel, summed over the batches of a file
 * (0 for a size query). */
gbwt_hip_status gbwt_hip_last_tags_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *plan_ms, float *gather_ms);

/* ---- suffix array and BWT of a text --------------------------------------------------------------------------------------------------
 * What stands between gbz-extract's two modes: `sequences` writes a text, `tag-array` reads `base`.sa, a suffix array of it, and counts the
 * runs of `base`.bwt (src/bin/gbz-extract.rs:321-344, 373-406).  For a text T[0, n) of bytes, SA is the permutation of 0 .. n - 1 that
 * orders the suffixes T[i, n) as unsigned byte strings compared to the end of the text, straight through any endmarkers; a suffix that is
 * a proper prefix of another is the smaller one (a generic suffix sorter's order for T followed by an implicit smallest sentinel).  All
 * suffixes differ in length: the order is total, SA is unique, there is no tie-break.  BWT[i] = T[SA[i] - 1], and the sentinel byte of the
 * call where SA[i] == 0; *bwt_runs = the runs of BWT[0, n) as count_bwt_runs counts them (the first entry starts a run; 0 for n == 0).
 * Built on the device by prefix doubling over radix sorts that re-sort only the suffixes still tied.  Ranks and positions
 * are 32 bits inside: n > 2^32 - 2 is GBWT_HIP_UNSUPPORTED before any work; scratch (49 bytes per position and the temporary storage of the
 * sorts) beyond the free device memory is GBWT_HIP_CAPACITY with the bytes needed.  All scratch is freed before a call returns.
 *
 * gbwt_hip_suffix_array_text: any n bytes in host memory, no index: out_sa[n], out_bwt[n] (may be NULL), *bwt_runs (may be NULL).
 * sentinel: a byte value 0 .. 255. */
gbwt_hip_status gbwt_hip_suffix_array_text(int device, const void *text, uint64_t n, int sentinel, uint64_t *out_sa, uint8_t *out_bwt, uint64_t *bwt_runs);
/* The same over the caller's device buffers: d_text[n] is only read, d_sa[n] and d_bwt[n] (may be NULL) are written, nothing outside them.
 * The work is ordered on `stream` (a hipStream_t; NULL: the default stream) and done when the call returns. */
gbwt_hip_status gbwt_hip_suffix_array_text_device(int device, const void *d_text, uint64_t n, int sentinel, uint64_t *d_sa, uint8_t *d_bwt, void *stream, uint64_t *bwt_runs);

/* The suffix array of the text of paths (GBZ handles opened with GBWT_HIP_OPEN_EXTRACT): the text is that of
 * gbwt_hip_path_sequences_device(path_ids, n, forward, endmarker), made by that family on `ws`; endmarker -1 (none) .. 255, the guards of the
 * bases calls.  The sentinel of the BWT is the endmarker (0 without one).  The results stay on the workspace until the next such request:
 * d_sa[total] is directly a valid suffix array for gbwt_hip_tags_device on the same workspace. */
typedef struct {
    uint64_t *d_sa;      /* [total] */
    uint8_t *d_bwt;      /* [total] */
    uint64_t total;      /* the length of the text */
    uint64_t bwt_runs;
} gbwt_hip_suffix_array;
gbwt_hip_status gbwt_hip_path_suffix_array_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int endmarker,
                                                  gbwt_hip_suffix_array *out);
/* The same copied out: *total always receives the text length; out_sa == NULL and out_bwt == NULL is the size query, and the call that
 * repeats its request with buffers (capacity: entries either holds) only copies -- nothing is built twice. */
gbwt_hip_status gbwt_hip_path_suffix_array(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int endmarker, uint64_t *out_sa,
                                           uint8_t *out_bwt, uint64_t capacity, uint64_t *total, uint64_t *bwt_runs);
/* The files between the two modes: reads `base`.names as gbwt_hip_write_tag_array does (path ids, and the bases of every path against
 * the walk), takes the endmarker from the last byte of `base` where that file exists -- its size must be the text's -- and 0 otherwise, and
 * writes `base`.sa (little-endian u64: the entry `total`, then SA) and `base`.bwt (the byte T[total - 1], then BWT): the entry and the byte
 * of the implicit sentinel in front, which gbwt_hip_write_tag_array(base, sa_skip = 1) and `gbz-extract -m tag-array -v` skip.  A `base`.sa
 * and a `base`.bwt that exist are removed once the arguments are through: neither file stays behind a failure, its own or an earlier call's. */
gbwt_hip_status gbwt_hip_write_suffix_array(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const char *base_path, uint64_t *bwt_runs);
/* The last suffix array built on `ws`, or with ws == NULL by a gbwt_hip_suffix_array_text* call of this process.  A round sorts the
 * active set -- the suffixes whose rank is still shared -- once: active[0] is its size behind the sort of the first keys (7 bytes),
 * active[k] behind round k, which compares 7 * 2^k bytes; rounds = the k that left it empty (entries past 63 are not kept).  round_ms[k]:
 * device time of that sort and its renumbering (round_ms[0]: the first keys'), by HIP events like text_ms (the bases of the paths, or
 * the upload of a host text), pack_ms, rank_ms (all rounds) and output_ms.  planned_scratch_bytes: what the plan promised for
 * peak_scratch_bytes, the most the ranking held at once. */
typedef struct {
    uint64_t n, peak_scratch_bytes, planned_scratch_bytes, bwt_runs;
    uint64_t active[64];
    uint32_t rounds, rank_bits;
    float text_ms, pack_ms, rank_ms, output_ms;
    float round_ms[64];
} gbwt_hip_suffix_array_info;
gbwt_hip_status gbwt_hip_last_suffix_array_info(const gbwt_hip_workspace *ws, gbwt_hip_suffix_array_info *out);

/* ---- FM-index over a text: count and locate patterns ------------------------------------------------------------------------------------
 * What the chain `sequences` -> suffix array -> tags is built for: "where in the graph does this string occur" is a backward search of the
 * pattern over the BWT of the haplotype texts, and the tags of the resulting SA range.  The reference has no FM-index; the contract is that
 * of the suffix array above: T[0, n) of arbitrary bytes, suffixes compared straight through endmarkers, a proper prefix first.  A pattern P
 * occurs at i when T[i, i + |P|) == P; its occurrences are the SA range [lo, hi), hi - lo of them.  A pattern that does not occur -- one
 * that holds a byte T lacks among them -- has the range (0, 0); the empty pattern has (0, n).
 *
 * The index is built on the device from T and SA: a code table for the sigma distinct bytes of T, C[c] = text bytes smaller
 * than c, and the BWT of n + 1 rows -- row 0 is the empty suffix, whose BWT byte is T[n - 1]; row j + 1 is SA row j -- in blocks with the
 * occurrences of every symbol in front of each block.  The row with SA[j] == 0 (`primary`) shows the call's sentinel in a BWT file; the
 * sentinel may equal a byte of T and never counts as one.  sigma <= 8 (endmarker, A, C, G, T, N): a block is one 128-byte line of eight
 * u32 counts and 96 BWT symbols, and one rank reads one line; larger alphabets: 256 symbols per block and the counts beside them.  Unless
 * built with GBWT_HIP_FM_COUNT_ONLY the index holds SA as u32 (n <= 2^32 - 2, else GBWT_HIP_UNSUPPORTED before any work).  Scratch beyond
 * the free device memory is GBWT_HIP_CAPACITY with the bytes needed; all scratch is freed before a build returns.
 *
 * An object serves ONE HOST THREAD AT A TIME: its requests run on a stream of its own, and their results stay in it until its next request. */
typedef struct gbwt_hip_fm_index gbwt_hip_fm_index;    /* opaque */
#define GBWT_HIP_FM_COUNT_ONLY 1u                       /* flags: no suffix array in the index; locate is GBWT_HIP_UNSUPPORTED */

/* Any n bytes in host memory.  sentinel: a byte value 0 .. 255 (the BWT byte in front of suffix 0; it changes no answer). */
gbwt_hip_status gbwt_hip_fm_build_text(int device, const void *text, uint64_t n, int sentinel, uint32_t flags, gbwt_hip_fm_index **out);
/* The same over the caller's device buffers, only read: d_text[n], and d_sa[n], the suffix array of gbwt_hip_suffix_array_text_device --
 * or NULL: the call makes it (its scratch: 8 n bytes and that call's).  A d_sa with a value outside the text or without an entry 0 is
 * GBWT_HIP_INVALID_DATA.  The build is ordered on `stream` (a hipStream_t; NULL: the default stream) and done when the call returns. */
gbwt_hip_status gbwt_hip_fm_build_text_device(int device, const void *d_text, uint64_t n, int sentinel, const uint64_t *d_sa, uint32_t flags, void *stream, gbwt_hip_fm_index **out);
/* The index of the text of paths: text and suffix array are those of gbwt_hip_path_suffix_array_device(path_ids, n, endmarker) on `ws`
 * (endmarker 0 .. 255: the tags count one behind every path).  The object remembers the handle, the path ids and the endmarker for
 * gbwt_hip_fm_graph_positions; it must be closed before the handle.
 * path_ids may stand in any order and may name an id more than once: every entry of the list is a row of the text with its own endmarker,
 * and two entries of one id are two copies of its bases -- a pattern occurs in both, their tags are equal, and the segment of a chain (its
 * `path`, the rank in the list) and its text offsets alone tell them apart.  The endmarker may be a byte that is also a base (65): the text
 * is what gbwt_hip_path_sequences writes, so a pattern or a seed can then occur across a path's end; such an occurrence is counted and
 * located like any other, the tag of an occurrence that starts on an endmarker byte is 0 whatever the byte is, and a chain still never
 * joins matches of different segments. */
gbwt_hip_status gbwt_hip_path_fm_index(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int endmarker, uint32_t flags,
                                       gbwt_hip_fm_index **out);
void gbwt_hip_fm_close(gbwt_hip_fm_index *fm);

/* block_rows: BWT symbols per block (96 packed, 256 plain); primary: the SA row with SA[i] == 0; index_bytes: what the object keeps for
 * the index (planned_index_bytes: what the plan promised), sa_bytes of it the suffix array (0 when count-only); peak_scratch_bytes /
 * planned_scratch_bytes: the build's own scratch (the ranking of a suffix array made by the build comes on top: see above).  Phase times
 * of the build by HIP events: suffix_array_ms (0 where the caller brought it), histogram_ms, codes_ms (the BWT symbols into the blocks),
 * counts_ms (per block, and their sums across blocks), fill_ms, narrow_ms (SA to u32).  queries: the requests computed so far -- a call that
 * repeats the request whose rows the object holds computes nothing and does not count; last_*: the patterns, backward steps (one per
 * pattern byte consumed), values in the rows, and the kernel times of the last computed request (count: the search; fill: scan and rows). */
typedef struct {
    uint64_t n, sigma, block_rows, blocks, primary, index_bytes, planned_index_bytes, sa_bytes, peak_scratch_bytes, planned_scratch_bytes;
    uint64_t queries, last_patterns, last_steps, last_total;
    uint32_t packed, count_only, path_level, reserved;
    float suffix_array_ms, histogram_ms, codes_ms, counts_ms, fill_ms, narrow_ms, last_count_ms, last_fill_ms;
} gbwt_hip_fm_index_info;
gbwt_hip_status gbwt_hip_fm_info(const gbwt_hip_fm_index *fm, gbwt_hip_fm_index_info *out);

/* Queries.  Patterns are a CSR: pattern k is bytes[offsets[k], offsets[k + 1]), offsets[m + 1] ascending (GBWT_HIP_BAD_ARGUMENT otherwise, before
 * any device work in the host forms).  One lane per pattern reads it backward and leaves once its range is empty.
 *
 * gbwt_hip_fm_count: ranges[2 k], ranges[2 k + 1] = (lo, hi) of pattern k.
 * gbwt_hip_fm_locate: row k = SA[lo_k .. hi_k) in SA order: out_offsets[m + 1] and *total always; positions == NULL is the size query, and the
 * call that repeats its request with a buffer (capacity: entries it holds; too few: GBWT_HIP_CAPACITY with *total) only copies -- nothing is
 * searched twice.  GBWT_HIP_UNSUPPORTED on a count-only index.
 * gbwt_hip_fm_graph_positions (an object of gbwt_hip_path_fm_index, with the handle it was made from and a workspace of it; anything else
 * is GBWT_HIP_BAD_ARGUMENT): the located positions go to gbwt_hip_tags_device on `ws` without leaving the device: row k = the tags of the
 * occurrences' first bases in SA order -- ((node << 11) | (orientation << 10)) + offset, 0 where an occurrence starts on an endmarker --,
 * or with unique == 1 the distinct tags ascending (sorted on the device; at most 2^31 - 1 positions in such a request).  Same protocol.
 * Any workspace of the handle serves, a different one in every call if need be, and requests for tags, bases or suffix arrays of other
 * paths on that workspace between two calls change no answer: the call asks the tags family for the object's own path ids each time. */
gbwt_hip_status gbwt_hip_fm_count(gbwt_hip_fm_index *fm, const uint64_t *offsets, const void *bytes, uint64_t m, uint64_t *ranges);
gbwt_hip_status gbwt_hip_fm_locate(gbwt_hip_fm_index *fm, const uint64_t *offsets, const void *bytes, uint64_t m, uint64_t *out_offsets, uint64_t *positions, uint64_t capacity,
                                   uint64_t *total);
gbwt_hip_status gbwt_hip_fm_graph_positions(gbwt_hip_fm_index *fm, const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *offsets, const void *bytes, uint64_t m,
                                            int unique, uint64_t *out_offsets, uint64_t *tags, uint64_t capacity, uint64_t *total);
/* The device forms: d_offsets[m + 1] and d_bytes[bytes] are in HBM and complete when the call is made (offsets that descend or exceed
 * `bytes` are GBWT_HIP_BAD_ARGUMENT, found by the kernel; nothing outside d_bytes[0, bytes) is read).  The results stay in HBM, owned by
 * the object, until its next request: d_ranges[2 m] for all three; d_offsets[m + 1] and d_values[total] -- positions, or tags -- for
 * locate and graph positions (NULL, total 0 for count). */
typedef struct {
    const uint64_t *d_offsets;   /* [m + 1] */
    const uint64_t *d_values;    /* [total] */
    const uint64_t *d_ranges;    /* [2 m] */
    uint64_t total, m;
} gbwt_hip_fm_located;
gbwt_hip_status gbwt_hip_fm_count_device(gbwt_hip_fm_index *fm, const uint64_t *d_offsets, const void *d_bytes, uint64_t m, uint64_t bytes, gbwt_hip_fm_located *out);
gbwt_hip_status gbwt_hip_fm_locate_device(gbwt_hip_fm_index *fm, const uint64_t *d_offsets, const void *d_bytes, uint64_t m, uint64_t bytes, gbwt_hip_fm_located *out);
gbwt_hip_status gbwt_hip_fm_graph_positions_device(gbwt_hip_fm_index *fm, const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *d_offsets, const void *d_bytes,
                                                   uint64_t m, uint64_t bytes, int unique, gbwt_hip_fm_located *out);

/* ---- Seeds of reads: maximal exact matches on the FM-index, on both strands -----------------------------------------------
 * A read rarely occurs as a whole; what a mapper asks is which pieces of it occur.  For a read P[0, L) of arbitrary bytes and an end e in
 * 1 .. L, s(e) is the smallest s <= e such that P[s, e) occurs in the text ("occurs" as gbwt_hip_fm_count means it: bytes are bytes; s(e) ==
 * e where P[e - 1] does not occur).  s never decreases as e grows.  A SEED is [s(e), e) with e - s(e) >= max(min_length, 1) and (e == L or
 * s(e + 1) > s(e)): exactly the occurring substrings of the read that no longer occurring substring of the read contains.  A seed carries
 * start, end, strand and the SA range [lo, hi) of P[start, end) in gbwt_hip_fm_count's coordinates; the seeds of a strand are listed with
 * starts and ends ascending.
 *
 * STRANDS: GBWT_HIP_STRAND_FORWARD searches the read as given (no case folding); GBWT_HIP_STRAND_REVERSE searches
 * support::reverse_complement of it (src/support.rs:87-110: A/C/G/T in either case to the upper-case complement, every other byte to N),
 * computed on the device, and its seeds are in the coordinates of the reverse-complemented read.  A read's row holds its forward seeds,
 * then its reverse seeds.
 *
 * HITS (max_occurrences > 0): one row per seed, in seed order: SA[lo, hi) in SA order where hi - lo <= max_occurrences, an empty row where
 * the seed occurs more often (it is still reported, and its range says how often).  gbwt_hip_fm_seed_graph_positions gives the rows as
 * tags through gbwt_hip_tags_device, as gbwt_hip_fm_graph_positions does, not uniqued.  A count-only index finds seeds and refuses hits
 * with GBWT_HIP_UNSUPPORTED.
 *
 * The search reads every read at the ends L, L - K, L - 2K, .. first (K = stride of the info) and between two of these only where the start
 * moved.  Its scratch is a function of (reads, read bytes, strands, hits); more than the free device memory is GBWT_HIP_CAPACITY with the
 * bytes needed, before the first kernel; all of it is freed before the call returns. */
#define GBWT_HIP_STRAND_FORWARD 1u
#define GBWT_HIP_STRAND_REVERSE 2u
#define GBWT_HIP_STRAND_BOTH 3u
typedef struct {
    uint32_t min_length;         /* seeds shorter than this are left out (0 counts as 1) */
    uint32_t strands;            /* 1 forward, 2 reverse, 3 both */
    uint64_t max_occurrences;    /* 0: no hits */
    uint32_t flags, reserved;    /* 0 */
} gbwt_hip_fm_seed_options;      /* NULL = {1, 3, 0, 0, 0} */
typedef struct {
    uint64_t lo, hi;
    uint32_t start, end;
    uint32_t strand, reserved;
} gbwt_hip_fm_seed;              /* 32 bytes */
/* The last computed seeds request of an object.  stride: K; anchors / refined_ends: the ends searched first / in between; steps: backward
 * steps (as last_steps of gbwt_hip_fm_index_info); idle_share: 1 - steps / (64 x the sum over the waves of the search of their longest lane):
 * the lane-steps a wave spent waiting for its longest lane; over_max: seeds with more than max_occurrences occurrences (their rows are
 * empty); planned / peak scratch bytes; HIP-event times of the anchor, refine, emit and hits phases. */
typedef struct {
    uint64_t requests, reads, read_bytes, anchors, refined_ends, steps, seeds, hits, over_max, planned_scratch_bytes, peak_scratch_bytes;
    uint32_t stride, strands;
    float idle_share, anchor_ms, refine_ms, emit_ms, hits_ms, reserved;
} gbwt_hip_fm_seed_info;
gbwt_hip_status gbwt_hip_fm_last_seed_info(const gbwt_hip_fm_index *fm, gbwt_hip_fm_seed_info *out);

/* Reads are a CSR as the patterns of the queries above.  out_read_offsets[m + 1], *total_seeds (and, with max_occurrences > 0,
 * *total_hits) always; seeds == NULL (and hits == NULL) is the size query, and the call that repeats its request with buffers only copies.
 * With hits, out_hit_offsets[*total_seeds + 1] is written together with the seeds.  A capacity that is too small is GBWT_HIP_CAPACITY with
 * the totals set and nothing written.  Checked before any device work, in this order: null outputs; null or descending offsets; strands
 * outside 1 .. 3; non-zero flags / reserved; then the object. */
gbwt_hip_status gbwt_hip_fm_seeds(gbwt_hip_fm_index *fm, const uint64_t *offsets, const void *bytes, uint64_t m, const gbwt_hip_fm_seed_options *opts, uint64_t *out_read_offsets,
                                  gbwt_hip_fm_seed *seeds, uint64_t seed_capacity, uint64_t *total_seeds, uint64_t *out_hit_offsets, uint64_t *hits, uint64_t hit_capacity,
                                  uint64_t *total_hits);
gbwt_hip_status gbwt_hip_fm_seed_graph_positions(gbwt_hip_fm_index *fm, const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *offsets, const void *bytes, uint64_t m,
                                                 const gbwt_hip_fm_seed_options *opts, uint64_t *out_read_offsets, gbwt_hip_fm_seed *seeds, uint64_t seed_capacity,
                                                 uint64_t *total_seeds, uint64_t *out_hit_offsets, uint64_t *tags, uint64_t hit_capacity, uint64_t *total_hits);
/* The device forms (d_offsets[m + 1], d_bytes[bytes] as above): the rows stay in HBM, owned by the object, until its next seeds request.
 * d_hit_offsets / d_hits are NULL without hits. */
typedef struct {
    const uint64_t *d_read_offsets;      /* [m + 1] */
    const gbwt_hip_fm_seed *d_seeds;     /* [total_seeds] */
    const uint64_t *d_hit_offsets;       /* [total_seeds + 1] */
    const uint64_t *d_hits;              /* [total_hits]: text positions, or tags */
    uint64_t total_seeds, total_hits, m;
} gbwt_hip_fm_seed_rows;
gbwt_hip_status gbwt_hip_fm_seeds_device(gbwt_hip_fm_index *fm, const uint64_t *d_offsets, const void *d_bytes, uint64_t m, uint64_t bytes, const gbwt_hip_fm_seed_options *opts,
                                         gbwt_hip_fm_seed_rows *out);
gbwt_hip_status gbwt_hip_fm_seed_graph_positions_device(gbwt_hip_fm_index *fm, const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *d_offsets, const void *d_bytes,
                                                        uint64_t m, uint64_t bytes, const gbwt_hip_fm_seed_options *opts, gbwt_hip_fm_seed_rows *out);

/* ---- Chains of seeds: colinear chaining of a read's hits -------------------------------------------------------------------
 * Which placements of a read do its hits support, and how well?  An ITEM is one (read, strand) pair of a seeds request.  Every hit p of a
 * seed [start, end) of the item is a MATCH (y = p, x = start, w = end - start): only the hits a seeds request with the same min_length,
 * strands and max_occurrences reports (a seed with more occurrences contributes none).  The matches of an item are ordered by (y, x), and
 * the index of a match is its place in that order.  max_matches (0: no limit) caps an item: one with more matches yields no chains and
 * counts as skipped.  All of it is integer arithmetic: nothing is heuristic.
 *
 * SEGMENTS: on an index of a plain text every match has segment 0; on an index of paths the segment of a match is the rank k (in the
 * path_ids the index was made with) of the path whose bases and endmarker hold y.  A chain never joins matches of different segments; a
 * seed that runs through an endmarker belongs to the segment of its first byte.
 * PRECEDENCE: match j may precede match i of the same item when both have one segment, dy = y_i - y_j and dx = x_i - x_j are in
 * 1 .. max_gap, and d = |dy - dx| <= max_skew.
 * SCORES: c(j, i) = f(j) + min(w_i, dx, dy) - gap_cost * d, signed.  f(i) = w_i and pred(i) = none unless some admissible j has
 * c(j, i) > w_i: then f(i) is the largest such c and pred(i) the largest j that attains it.
 * PEELING: the matches are visited by (f descending, index ascending).  An unused match i starts a chain and walks i, pred(i), .., marking
 * each used and making it a member, until a match has no predecessor (base = 0) or its predecessor p is used (base = f(p); p is no
 * member).  The chain's score is f(i) - base; it is reported when score >= max(min_score, 1), and its members stay used either way.
 * ROWS: a read's row holds the chains of its forward strand, then those of its reverse strand, each in peeling order -- the first chain of
 * an item is its best --; the members of a chain are listed by ascending index.  Coordinates on the reverse strand are those of the
 * reverse-complemented read, as for seeds.
 *
 * A chains request is a seeds request with hits as text positions, followed by the chaining: afterwards the seeds rows of the object are
 * those of that request, and gbwt_hip_fm_seeds with the same arguments computes nothing.  The chaining's scratch is a function of (hits,
 * items); more than the free device memory is GBWT_HIP_CAPACITY with the bytes needed, before its first kernel; all of it is freed before
 * the call returns.  A request with 2^31 or more hits is GBWT_HIP_UNSUPPORTED. */
typedef struct {
    uint32_t max_gap, max_skew;      /* 0: 5000 / 500 -- conventions, not tuned values */
    uint32_t gap_cost, min_score;    /* gap_cost 0 is allowed (no penalty); min_score 0 counts as 1 */
    uint64_t max_matches;            /* per (read, strand); 0: no limit */
    uint32_t flags, reserved;        /* 0 */
} gbwt_hip_fm_chain_options;         /* NULL = all zero */
/* text_start / read_start: y / x of the first member; text_end / read_end: y + w / x + w of the last; matches: the members; path: the
 * segment (0 on an index of a plain text) */
typedef struct { uint64_t text_start, text_end; uint32_t read_start, read_end, score, matches, strand, path; } gbwt_hip_fm_chain;   /* 40 bytes */
typedef struct { uint64_t y; uint32_t x, w; } gbwt_hip_fm_chain_match;                                                             /* 16 bytes */
/* The last computed chains request of an object.  items: reads x strands; matches: those of the items not skipped; pairs: admissible
 * (j, i) evaluated; chains / chain_matches: reported chains and their members; tile_matches: the most matches of an item that the DP
 * kernel stages in LDS (larger items run over global memory; a constant of the build, set in every answer); path_offset_bytes: what an
 * index of paths keeps for the segments (not part of index_bytes); HIP-event times: seeds_ms (0 where the seeds step was answered from
 * the object's seeds rows), expand_ms, sort_ms, dp_ms, peel_ms, fill_ms. */
typedef struct {
    uint64_t requests, items, matches, skipped_items, pairs, chains, chain_matches, tile_matches, planned_scratch_bytes, peak_scratch_bytes, path_offset_bytes;
    float seeds_ms, expand_ms, sort_ms, dp_ms, peel_ms, fill_ms;
} gbwt_hip_fm_chain_info;
gbwt_hip_status gbwt_hip_fm_last_chain_info(const gbwt_hip_fm_index *fm, gbwt_hip_fm_chain_info *out);

/* Reads and seed options as gbwt_hip_fm_seeds takes them (max_occurrences == 0 is GBWT_HIP_BAD_ARGUMENT: chains need hits).
 * out_read_offsets[m + 1], *total_chains and *total_matches always; chains == NULL (and matches == NULL) is the size query, and the call
 * that repeats its request with buffers only copies.  out_match_offsets[*total_chains + 1] is written together with the chains.  A
 * capacity that is too small is GBWT_HIP_CAPACITY with the totals set and nothing written.  Checked before any device work, in this
 * order: null outputs; the reads; the seed options; the chain options (non-zero flags / reserved; max_gap or max_skew above 2^31 - 1;
 * gap_cost x max_skew >= 2^31); then the object (a count-only index is GBWT_HIP_UNSUPPORTED). */
gbwt_hip_status gbwt_hip_fm_chains(gbwt_hip_fm_index *fm, const uint64_t *offsets, const void *bytes, uint64_t m, const gbwt_hip_fm_seed_options *seed_opts,
                                   const gbwt_hip_fm_chain_options *chain_opts, uint64_t *out_read_offsets, gbwt_hip_fm_chain *chains, uint64_t chain_capacity, uint64_t *total_chains,
                                   uint64_t *out_match_offsets, gbwt_hip_fm_chain_match *matches, uint64_t match_capacity, uint64_t *total_matches);
/* The device form: the rows stay in HBM, owned by the object, until its next chains request. */
typedef struct {
    const uint64_t *d_read_offsets;              /* [m + 1] */
    const gbwt_hip_fm_chain *d_chains;           /* [total_chains] */
    const uint64_t *d_match_offsets;             /* [total_chains + 1] */
    const gbwt_hip_fm_chain_match *d_matches;    /* [total_matches] */
    uint64_t total_chains, total_matches, m;
} gbwt_hip_fm_chain_rows;
gbwt_hip_status gbwt_hip_fm_chains_device(gbwt_hip_fm_index *fm, const uint64_t *d_offsets, const void *d_bytes, uint64_t m, uint64_t bytes, const gbwt_hip_fm_seed_options *seed_opts,
                                          const gbwt_hip_fm_chain_options *chain_opts, gbwt_hip_fm_chain_rows *out);

/* ---- Alignments of chains: banded edit distance and CIGARs ----------------------------------------------------------------
 * A chain says which placement of a read its exact matches support; an alignment says how the read lies there: where it starts and ends
 * in the text, how many edits, and the CIGAR.  Integer arithmetic, nothing heuristic.  It needs the text, which the builds do not keep:
 *
 * THE TEXT.  gbwt_hip_fm_set_text / gbwt_hip_fm_set_text_device give the object a copy of n bytes in HBM (n != the n of the index:
 * GBWT_HIP_BAD_ARGUMENT; a byte histogram that is not the index's -- its code table and C -- : GBWT_HIP_INVALID_DATA.  One kernel pass: it
 * catches a wrong text cheaply and is no proof of equality).  gbwt_hip_fm_keep_path_text, on an object of gbwt_hip_path_fm_index with the
 * handle it was made from and a workspace of it (the checks of gbwt_hip_fm_graph_positions), asks the bases family on `ws` for the
 * object's own path ids with its endmarker and copies the text device to device.  A second call replaces the text; gbwt_hip_fm_close
 * frees it.  The text is no part of index_bytes / planned_index_bytes: gbwt_hip_fm_last_align_info reports it as text_bytes.
 *
 * WHICH CHAINS.  Per item (read, strand) the first max_alignments chains in peeling order (0: all).  A read's row holds the alignments of
 * its forward strand, then those of its reverse strand, in chain order; every considered chain yields exactly one row, whatever its status.
 * THE READ AND THE TEXT.  P[0, L) is the read as the strand of the chain sees it (the reverse complement is computed on the device); T is
 * the kept text.  Bytes are bytes: no case folding, and N == N.
 * BOUNDS.  [lo, hi) = [0, n) on an index of a plain text; on an index of paths the bases of the chain's `path` without its endmarker:
 * lo = path_offsets[path], hi = path_offsets[path + 1] - 1.  An alignment never touches an endmarker byte, whatever its value.
 * THE BAND.  A member (y, x, w) of the chain lies on the diagonal d = y - x (signed 64-bit).  d0 = min d - band, d1 = max d + band,
 * W = d1 - d0 + 1.  W > max_width: status GBWT_HIP_ALIGN_WIDE, nothing is computed, the CIGAR row is empty.
 * CELLS.  H(i, j) for 0 <= i <= L and j = i + d, d0 <= d <= d1; only cells with lo <= j <= hi exist, every other one is unreachable.
 * H(0, j) = 0 for every existing cell of row 0: the start in the text is free.  For i >= 1, H(i, j) is the smallest candidate that comes
 * from an existing, reachable cell: the diagonal H(i - 1, j - 1) + (P[i - 1] != T[j - 1]); the insertion (a read byte without a text
 * byte) H(i - 1, j) + 1; the deletion (a text byte without a read byte) H(i, j - 1) + 1.  The direction of the cell is the first of
 * (diagonal, insertion, deletion) that attains the minimum; a cell without a candidate is unreachable.
 * THE RESULT.  edit_distance = the smallest H(L, j) over the band, text_end = the smallest j that attains it.  No reachable cell in row L
 * (the read overhangs its path by more than the band allows): status GBWT_HIP_ALIGN_NONE, edit_distance 0xFFFFFFFF, text_start =
 * text_end = 0, an empty CIGAR row.
 * THE CIGAR.  The walk back starts at (L, text_end) and follows the directions until i == 0, where text_start = j.  The free start means
 * that no leading deletion occurs, the smallest end that no trailing one does.  The operations stand in read order, run-length encoded as
 * u32 = (length << 4) | op with BAM's codes: I = 1, D = 2, '=' = 7, X = 8.
 *
 * An alignments request is a chains request followed by the alignment: afterwards the chains rows and the seeds rows of the object are
 * those of that request, and gbwt_hip_fm_chains / gbwt_hip_fm_seeds with the same arguments compute nothing.  The alignment's scratch is a
 * function of (items, considered chains, the directions that do not fit the LDS tile, the CIGAR bound of 2 L entries per computed
 * alignment); more than the free device memory is GBWT_HIP_CAPACITY with the bytes needed, before the first kernel that aligns; all of it
 * is freed before the call returns.  A computed alignment of a read of 2^28 bytes or more is GBWT_HIP_UNSUPPORTED. */
gbwt_hip_status gbwt_hip_fm_set_text(gbwt_hip_fm_index *fm, const void *text, uint64_t n);
gbwt_hip_status gbwt_hip_fm_set_text_device(gbwt_hip_fm_index *fm, const void *d_text, uint64_t n, void *stream);
gbwt_hip_status gbwt_hip_fm_keep_path_text(gbwt_hip_fm_index *fm, const gbwt_hip_index *index, gbwt_hip_workspace *ws);

typedef struct {
    uint32_t band, max_width;        /* band is taken as given (0: the chain's own diagonals); max_width 0: 256; both at most 1024 */
    uint64_t max_alignments;         /* per (read, strand); 0: all chains */
    uint32_t flags, reserved;        /* 0 */
} gbwt_hip_fm_align_options;         /* 24 bytes; NULL = {16, 256, 0, 0, 0} */
/* chain: the index of the chain in the chains rows of the same request; width: W, set for every status */
typedef struct { uint64_t text_start, text_end; uint32_t chain, edit_distance, width, status, strand, path; } gbwt_hip_fm_alignment;  /* 40 bytes */
#define GBWT_HIP_ALIGN_OK 0u
#define GBWT_HIP_ALIGN_WIDE 1u
#define GBWT_HIP_ALIGN_NONE 2u
/* The last computed alignments request of an object.  items: reads x strands; chains: those considered; alignments: the rows (one per
 * considered chain); wide / unreachable: rows of status WIDE / NONE; cells: the sum of (L + 1) x W over the computed ones (every status
 * but WIDE); cigar_ops: CIGAR entries; lds_alignments / global_alignments: computed alignments whose directions went to the LDS tile / to
 * scratch in HBM; tile_bytes: the tile -- directions of L x ceil(W / 16) x 4 bytes fit up to it -- and text_bytes: the kept text; both
 * are set in every answer; HIP-event times: chains_ms (0 where the chains step was answered from the object's chains rows), select_ms
 * (the considered chains, their bands and sizes), dp_ms, trace_ms (0: the walk back runs inside the DP kernel and is part of dp_ms),
 * rows_ms. */
typedef struct {
    uint64_t requests, items, chains, alignments, wide, unreachable, cells, cigar_ops, lds_alignments, global_alignments, tile_bytes, text_bytes, planned_scratch_bytes,
        peak_scratch_bytes;
    float chains_ms, select_ms, dp_ms, trace_ms, rows_ms, reserved;
} gbwt_hip_fm_align_info;
gbwt_hip_status gbwt_hip_fm_last_align_info(const gbwt_hip_fm_index *fm, gbwt_hip_fm_align_info *out);

/* Reads, seed options and chain options as gbwt_hip_fm_chains takes them.  out_read_offsets[m + 1], *total_alignments and *total_cigars
 * always; alignments == NULL (and cigars == NULL) is the size query, and the call that repeats its request with buffers only copies.
 * out_cigar_offsets[*total_alignments + 1] is written together with the alignments.  A capacity that is too small is GBWT_HIP_CAPACITY
 * with the totals set and nothing written.  Checked before any device work, in this order: null outputs; the reads; the seed options; the
 * chain options; the align options (non-zero flags / reserved; max_width or band above 1024); then the object (a count-only index is
 * GBWT_HIP_UNSUPPORTED, and so is one without a text: see gbwt_hip_fm_set_text and gbwt_hip_fm_keep_path_text). */
gbwt_hip_status gbwt_hip_fm_alignments(gbwt_hip_fm_index *fm, const uint64_t *offsets, const void *bytes, uint64_t m, const gbwt_hip_fm_seed_options *seed_opts,
                                       const gbwt_hip_fm_chain_options *chain_opts, const gbwt_hip_fm_align_options *align_opts, uint64_t *out_read_offsets,
                                       gbwt_hip_fm_alignment *alignments, uint64_t capacity, uint64_t *total_alignments, uint64_t *out_cigar_offsets, uint32_t *cigars,
                                       uint64_t cigar_capacity, uint64_t *total_cigars);
/* The device form: the rows stay in HBM, owned by the object, until its next alignments request. */
typedef struct {
    const uint64_t *d_read_offsets;              /* [m + 1] */
    const gbwt_hip_fm_alignment *d_alignments;   /* [total_alignments] */
    const uint64_t *d_cigar_offsets;             /* [total_alignments + 1] */
    const uint32_t *d_cigars;                    /* [total_cigars] */
    uint64_t total_alignments, total_cigars, m;
} gbwt_hip_fm_alignment_rows;
gbwt_hip_status gbwt_hip_fm_alignments_device(gbwt_hip_fm_index *fm, const uint64_t *d_offsets, const void *d_bytes, uint64_t m, uint64_t bytes,
                                              const gbwt_hip_fm_seed_options *seed_opts, const gbwt_hip_fm_chain_options *chain_opts, const gbwt_hip_fm_align_options *align_opts,
                                              gbwt_hip_fm_alignment_rows *out);

/* ---- graph topology: weakly connected components, contig path selection -------------------------------------------------------------
 * GBZ::weakly_connected_components (src/gbz.rs:570-598; known answer src/gbz/tests.rs:503-518): the node ids of the graph that the GBWT
 * records describe, partitioned by "joined through an edge, whatever the orientations" (the successors and predecessors of both
 * orientations of every node, EdgeIter with the ENDMARKER edge skipped, src/gbz.rs:819-855), the components in order of their smallest
 * node id, the nodes ascending inside (DisjointSets::extract, src/support.rs:1551-1576).  A node exists by GBZ::has_node (src/gbz.rs:286-289):
 * its forward record is non-empty and holds an edge.
 *
 * Components belong to the index.  They are computed on the device from the record bytes, the record starts and the endmarker -- what
 * EVERY handle keeps, whatever its GBWT_HIP_OPEN_* flags, GBZ or bare GBWT -- by the first call below on a handle (once, whichever
 * thread asks first; an open never makes them), stay in HBM (4 bytes per node slot, the CSR and 4 bytes per path) and are counted in
 * gbwt_hip_memory_usage's index_device_bytes from then on.
 *
 * NODE SLOTS: slot s stands for node id min_node + s, min_node = GBZ::min_node (src/gbz.rs:274-276), slots = max_node + 1 - min_node
 * (GBZ::max_node, :280-282): the domain of the reference's DisjointSets.
 *
 * gbwt_hip_components_device: the device-resident view, valid while the handle is open: d_component[slots] = component of the node of
 * every slot (UINT32_MAX for a node that does not exist); component c = d_nodes[d_offsets[c] .. d_offsets[c + 1]) (u32 node ids);
 * d_path_component[paths] as gbwt_hip_path_components. */
typedef struct {
    const uint32_t *d_component; const uint64_t *d_offsets; const uint32_t *d_nodes; const uint32_t *d_path_component;
    uint64_t min_node, slots, components, nodes, paths;
} gbwt_hip_components;
gbwt_hip_status gbwt_hip_components_device(const gbwt_hip_index *index, gbwt_hip_components *out);
/* GBZ::weakly_connected_components as a host CSR: out_offsets[components + 1], out_nodes[nodes] (node ids).  *components and *nodes
 * always receive the counts; out_offsets == NULL and out_nodes == NULL is a size query; offsets_capacity < components + 1 or
 * nodes_capacity < nodes -> GBWT_HIP_CAPACITY. */
gbwt_hip_status gbwt_hip_weakly_connected_components(const gbwt_hip_index *index, uint64_t *out_offsets, uint64_t offsets_capacity, uint64_t *out_nodes,
                                                     uint64_t nodes_capacity, uint64_t *components, uint64_t *nodes);
/* out[k] = the component of path path_ids[k]: that of the first node of GBZ::path(id, Forward) (src/gbz.rs:461-466; what select_paths looks
 * up, src/bin/gbz-extract.rs:243-246, 253-256), UINT32_MAX for an empty path (`if let Some(..)` there).  Path p is sequence 2 p of a
 * bidirectional index (support::encode_path), sequence p of a unidirectional one.  An id >= paths -> GBWT_HIP_BAD_ARGUMENT. */
gbwt_hip_status gbwt_hip_path_components(const gbwt_hip_index *index, const uint64_t *path_ids, uint64_t n, uint32_t *out);
/* Device time (HIP events) of the build that made the components of this handle, and its launches: hook = the passes over the edge lists
 * of all records, jump = the pointer-jumping passes over the labels, shape = component numbers, CSR and path components.
 * GBWT_HIP_BAD_ARGUMENT before the components have been made. */
typedef struct { float hook_ms, jump_ms, shape_ms; uint32_t hook_launches, jump_launches, shape_launches; } gbwt_hip_components_times;
gbwt_hip_status gbwt_hip_last_components_ms(const gbwt_hip_index *index, gbwt_hip_components_times *out);
/* select_paths of gbz-extract (src/bin/gbz-extract.rs:196-264), for an index with metadata and path names: contig == NULL selects every
 * path of the metadata; otherwise the ascending ids of every path whose first node lies in a component in which a path with contig name
 * `contig` starts.  *total always receives the number of paths; out_path_ids == NULL is a size query; capacity < total ->
 * GBWT_HIP_CAPACITY.  GBWT_HIP_BAD_ARGUMENT with the reference's messages (:212-224): "Cannot select a contig without contig names",
 * "The graph does not contain contig NAME", "The graph does not contain any paths for contig NAME"; and without metadata or path names. */
gbwt_hip_status gbwt_hip_select_paths(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const char *contig, uint64_t *out_path_ids, uint64_t capacity,
                                      uint64_t *total);
/* gbz-extract -c contig -o path (extract_sequences, src/bin/gbz-extract.rs:266-294): gbwt_hip_write_sequences for the paths
 * gbwt_hip_select_paths selects, byte for byte. */
gbwt_hip_status gbwt_hip_write_sequences_contig(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const char *path, const char *contig, int endmarker);

/* ---- the graph: nodes, edges, segments, links, and the H-/S-/L-lines of a GFA file ----------------------------------------------------
 * An EDGE or LINK is reported as 2 * id + orientation (support::encode_node, src/support.rs:155-157; orientation 0 = forward), as uint64_t.
 * Batched requests give a CSR: row k = out[out_offsets[k] .. out_offsets[k + 1]), valid[k] = 1 where the reference returns an iterator
 * (an empty one included) and 0, with an empty row, where it returns None.  A request is never refused for an id it does not know.
 * The size query and GBWT_HIP_CAPACITY work as in gbwt_hip_follow: out_offsets[n + 1], valid[n] and *total are always filled; the rows are
 * copied when out_edges != NULL and capacity >= *total.  The device-resident forms leave the CSR in the workspace, valid until the next
 * edges / links request on it.
 *
 * gbwt_hip_node_ids: GBZ::node_iter (src/gbz.rs:312-317): the ids of the nodes for which GBZ::has_node holds (src/gbz.rs:286-289: the
 * forward record is non-empty and holds an edge), ascending.  Any handle.  out == NULL is a size query. */
gbwt_hip_status gbwt_hip_node_ids(const gbwt_hip_index *index, uint64_t *out, uint64_t capacity, uint64_t *total);
/* GBZ::successors (predecessors == 0, src/gbz.rs:327-335) / GBZ::predecessors (src/gbz.rs:345-353) of node_ids[k] in orientations[k]
 * (EdgeIter, src/gbz.rs:819-870): the edges of the record of the oriented node -- of the flipped node for predecessors, every edge then
 * flipped -- in record order, a leading ENDMARKER edge left out.  valid[k] = 0 where !has_node(node_id) -- id 0, below min_node and at or
 * above alphabet_size / 2 included -- or the record of the oriented node is absent or empty (BWT::record -> None, src/bwt.rs:124-131; the
 * reverse records of a unidirectional index).  Any handle, whatever its GBWT_HIP_OPEN_* flags, a bare GBWT included. */
typedef struct { const uint64_t *d_offsets; const uint64_t *d_edges; const uint8_t *d_valid; uint64_t total; uint64_t n; } gbwt_hip_edge_rows;
gbwt_hip_status gbwt_hip_edges(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *node_ids, const uint8_t *orientations, uint64_t n,
                               int predecessors, uint64_t *out_offsets, uint64_t *out_edges, uint64_t capacity, uint64_t *total, uint8_t *valid);
gbwt_hip_status gbwt_hip_edges_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *node_ids, const uint8_t *orientations,
                                      uint64_t n, int predecessors, gbwt_hip_edge_rows *out);
/* GBZ::segment_iter (src/gbz.rs:381-390, SegmentIter 919-935): the ids of the segments whose first node exists, ascending.  *total = 0
 * without a node-to-segment translation (the reference: None).  A GBZ handle; out_ids == NULL is a size query. */
gbwt_hip_status gbwt_hip_segments(const gbwt_hip_index *index, uint64_t *out_ids, uint64_t capacity, uint64_t *total);
/* GBZ::node_to_segment (src/gbz.rs:370-376): out_segments[k] = the id of the segment that holds node_ids[k]; valid[k] = 0 without a
 * translation or without the node. */
gbwt_hip_status gbwt_hip_node_segments(const gbwt_hip_index *index, const uint64_t *node_ids, uint64_t n, uint64_t *out_segments, uint8_t *valid);
/* GBZ::segment_successors / segment_predecessors (src/gbz.rs:402-440, LinkIter 988-1005) of segment_ids[k] in orientations[k]: the edges of
 * the boundary node -- nodes.end - 1 for forward successors and reverse predecessors, nodes.start otherwise -- each node replaced by its
 * segment (Graph::node_to_segment, src/graph.rs:186-198); the row ends in front of the first listed node without a segment, where
 * LinkIter::next returns None.  valid[k] = 0 without a translation, for a segment id out of range, and where successors / predecessors of
 * the boundary node is None.  A GBZ opened with GBWT_HIP_OPEN_GFA (the translation tables in HBM); otherwise GBWT_HIP_BAD_ARGUMENT. */
gbwt_hip_status gbwt_hip_links(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *segment_ids, const uint8_t *orientations, uint64_t n,
                               int predecessors, uint64_t *out_offsets, uint64_t *out_links, uint64_t capacity, uint64_t *total, uint8_t *valid);
gbwt_hip_status gbwt_hip_links_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *segment_ids, const uint8_t *orientations,
                                      uint64_t n, int predecessors, gbwt_hip_edge_rows *out);
/* The graph of a GFA file as gbunzip writes it (write_gfa_header, write_segments, write_links, src/bin/gbunzip.rs:193-332), formatted on the
 * device: d_text = the H-line (header_bytes; with RS:Z: when the GBWT has the tag reference_samples), the S-lines (segment_bytes,
 * `segments` lines) and the L-lines (link_bytes, `links` lines; the canonical ones: from a forward node to >= its id, from a reverse node
 * to > its id or to the same id forward), byte for byte; node ids in decimal, or segment names with a translation.  A GBZ opened with
 * GBWT_HIP_OPEN_GFA; otherwise GBWT_HIP_BAD_ARGUMENT.  The first request of a handle uploads the node labels, as the first request for
 * bases does.  Sizes and offsets stay in the workspace: a later request formats again without sizing.  The text is valid until the next
 * graph lines request on the workspace. */
typedef struct { const char *d_text; uint64_t header_bytes, segment_bytes, link_bytes, segments, links; } gbwt_hip_graph_text;
gbwt_hip_status gbwt_hip_graph_lines_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws, gbwt_hip_graph_text *out);
/* The same text in host memory; *total = its bytes; out == NULL is a size query; capacity < *total -> GBWT_HIP_CAPACITY. */
gbwt_hip_status gbwt_hip_graph_lines(const gbwt_hip_index *index, gbwt_hip_workspace *ws, char *out, uint64_t capacity, uint64_t *total);
/* Device time (HIP events) of the last graph lines request: sizing (0 where the kept sizes were used), S-line fill, L-line fill. */
gbwt_hip_status gbwt_hip_last_graph_ms(const gbwt_hip_workspace *ws, float *size_ms, float *segments_ms, float *links_ms);

/* ---- reference positions (GBZ handles opened with GBWT_HIP_OPEN_GFA) --------------------------------------------------------------------
 * GBZ::reference_positions (src/gbz.rs:600-657, result type ReferencePath :1255-1266; known answer src/gbz/tests.rs:521-567): for a forward
 * path p (sequence 2 p) with nodes v_0 .. v_{m-1}, off_0 = 0 and off_{k+1} = off_k + sequence_len(node_id(v_k)), the path's length in bases
 * len = off_m and the KEPT visits i_0 = 0 (if m > 0), i_{j+1} = the first k > i_j with off_k >= off_{i_j} + interval (the sum saturates at
 * 2^64 - 1; interval = 0 keeps every visit), each as (off_k, Pos{v_k, o_k}) with Pos_0 = GBWT::start(2 p), Pos_{k+1} = GBWT::forward(Pos_k).
 * An empty path has len = 0 and no positions.  Base offsets and lengths are u64 throughout.
 *
 * The walk, the offsets, the selection (pointer doubling over the successor of every visit, no chain serial in the path length) and the LF
 * steps that carry the in-record offset all run on the device; scratch is 24 bytes per node of the requested paths on the workspace,
 * counted in workspace_device_bytes.  A request whose paths hold more than 2^32 - 1 nodes together is GBWT_HIP_UNSUPPORTED (positions are
 * indexed in 32 bits inside); scratch or results that do not fit in free device memory are GBWT_HIP_CAPACITY.  GBWT_HIP_UNSUPPORTED for a
 * bare GBWT (no node labels), GBWT_HIP_BAD_ARGUMENT for a handle opened without GBWT_HIP_OPEN_GFA; GBWT_HIP_DEVICE_ERROR when a walker
 * met another node than the extracted row holds (an inconsistent index). */
typedef struct { uint64_t path_id, len, first, count; } gbwt_hip_reference_path;   /* its positions: [first, first + count) of the request's */
typedef struct { uint64_t offset; gbwt_hip_pos pos; } gbwt_hip_reference_position; /* 24 bytes */
/* GBZ::reference_sample_names (src/gbz.rs:183-196): the names of the GBWT tag `reference_samples`, split at ' ', then (also_generic != 0)
 * `_gbwt_ref`, those that the metadata's sample dictionary holds, each followed by '\n', in out[0 .. *total).  Host only.  out == NULL is a
 * size query; capacity < *total -> GBWT_HIP_CAPACITY.  Without metadata: nothing (*total = 0). */
gbwt_hip_status gbwt_hip_reference_sample_names(const gbwt_hip_index *index, int also_generic, char *out, uint64_t capacity, uint64_t *total);
/* The reference paths (src/gbz.rs:609-629): the ids, ascending, of the paths whose sample is one of those names.  Host only.  *count always
 * receives their number; out_ids == NULL is a size query; capacity < *count -> GBWT_HIP_CAPACITY.  No reference samples, or no path names:
 * no paths, GBWT_HIP_OK.  No metadata: GBWT_HIP_BAD_ARGUMENT (the reference unwraps it). */
gbwt_hip_status gbwt_hip_reference_paths(const gbwt_hip_index *index, int also_generic, uint64_t *out_ids, uint64_t capacity, uint64_t *count);
/* The general form: any forward path ids, in the order given; a duplicate gets a row of its own; an id >= paths is GBWT_HIP_BAD_ARGUMENT.
 * d_paths[n] and d_positions[*total] stay in HBM on the workspace, valid until the next request for positions on it. */
gbwt_hip_status gbwt_hip_path_positions_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, uint64_t interval,
                                               const gbwt_hip_reference_path **d_paths, const gbwt_hip_reference_position **d_positions, uint64_t *total);
/* The same copied to host buffers: out_paths[n] (may be NULL), out_positions[*total]; out_positions == NULL is a size query,
 * positions_capacity < *total -> GBWT_HIP_CAPACITY (out_paths is filled all the same).  The fill call that repeats the request of a size
 * query does not compute again. */
gbwt_hip_status gbwt_hip_path_positions(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, uint64_t interval,
                                        gbwt_hip_reference_path *out_paths, gbwt_hip_reference_position *out_positions, uint64_t positions_capacity, uint64_t *total);
/* GBZ::reference_positions(interval): gbwt_hip_reference_paths(also_generic = 1) followed by gbwt_hip_path_positions.  *n_paths and *total
 * always receive the counts; out_paths == NULL and out_positions == NULL is a size query; paths_capacity < *n_paths or
 * positions_capacity < *total -> GBWT_HIP_CAPACITY. */
gbwt_hip_status gbwt_hip_reference_positions(const gbwt_hip_index *index, gbwt_hip_workspace *ws, uint64_t interval, gbwt_hip_reference_path *out_paths,
                                             uint64_t paths_capacity, uint64_t *n_paths, gbwt_hip_reference_position *out_positions, uint64_t positions_capacity,
                                             uint64_t *total);
/* Device time of the last request for positions on `ws` (HIP events): *walk_ms = the walk kernel of its extraction, *select_ms = label
 * lengths, scans, successors and the pointer-doubling rounds up to the host's wait for the total, *offsets_ms = the LF walk that carries the
 * in-record offsets and writes the positions. */
gbwt_hip_status gbwt_hip_last_positions_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *select_ms, float *offsets_ms);
/* Of the same request: the pointer-doubling rounds that marked something, and the kernels and scans it launched behind its extraction (a scan
 * counts one launch per piece of GBWT_HIP_SCAN_PIECE positions: one, short of 2^30 positions). */
gbwt_hip_status gbwt_hip_last_positions_rounds(const gbwt_hip_workspace *ws, uint32_t *rounds, uint32_t *launches);

/* ---- locate: the sequences behind a search state (any handle) ---------------------------------------------------------------------------
 * The C++ GBWT's locate(node, i) and locate(SearchState).  The reference has no counterpart: its README leaves "Locate queries" open and it
 * passes the document array samples through uninterpreted (src/gbwt.rs:416), so the contract is stated here.  A SEQUENCE ID is a GBWT
 * sequence id (2 * path + orientation in a bidirectional index).  Every BWT position (node, offset), offset < the length of the node's
 * record, is the visit of exactly one sequence: GBWT::start(id) followed by GBWT::forward meets every position once.
 *
 * gbwt_hip_locate_positions: ids[k] = the id of the sequence whose visit positions[k] is.  valid[k] = 0 and ids[k] = 0 where the node has no
 * record (node <= alphabet_offset -- the endmarker, node 0, included --, node >= alphabet_size, a node without a record) or the offset is
 * >= the record's length.
 * gbwt_hip_locate: for states[k] = (node, start, end), end exclusive, a CSR like the edge rows: row k = ids[offsets[k] .. offsets[k + 1]).
 *   unique == 0: end - start ids, the owner of offset start, start + 1, ... in that order; a sequence that visits the node several times
 *                appears several times.
 *   unique == 1: the same ids ascending, duplicates removed (what the C++ GBWT returns for locate(SearchState)).
 *   valid[k] = 0, with an empty row, where the node has no record, start >= end, or end exceeds the record's length; such a state never fails
 *   the batch.  unique other than 0 / 1 is GBWT_HIP_BAD_ARGUMENT.
 * The size query and GBWT_HIP_CAPACITY work as in gbwt_hip_edges: offsets[n + 1], valid[n] and *total are always filled; the ids are copied
 * when ids != NULL and capacity >= *total; the fill call that repeats the request of a size query does not compute again.
 *
 * The first locate call on a handle builds its LOCATE INDEX in HBM, from whichever workspace asks (once; other threads wait for it; it lives
 * as long as the handle and is counted in index_device_bytes): the sequence id of every position of the SAMPLED records -- a record is
 * sampled when a hash of its index falls below a threshold; GBWT_HIP_LOCATE_INTERVAL, read at open, is the expected number of records
 * between two sampled ones: default 64, 1 = every record, 0 = none -- and the last position of every sequence.  A query steps with LF from
 * its position until it stands on a sampled record or its sequence ends.  Limits, checked at the build: the sequences and every record's
 * length fit 32 bits (more than 2^31 - 1 sequences, or a record of 2^32 - 1 positions or more: GBWT_HIP_UNSUPPORTED).  A walk of the build
 * that does not fill every slot of the table exactly once is GBWT_HIP_INVALID_DATA, and nothing is kept.  A unique request is sorted in
 * pieces of at most 2^31 - 1 ids cut at row boundaries; a single row longer than that is GBWT_HIP_UNSUPPORTED.  A request waits for the
 * host once, for its total (a unique one a second time, for the total after the duplicates are gone). */
typedef struct { const uint64_t *d_offsets; const uint64_t *d_ids; const uint8_t *d_valid; uint64_t total; uint64_t n; } gbwt_hip_located;
gbwt_hip_status gbwt_hip_locate(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const gbwt_hip_state *states, uint64_t n, int unique, uint64_t *offsets,
                                uint64_t *ids, uint64_t capacity, uint64_t *total, uint8_t *valid);
/* The same rows left in HBM: d_offsets u64[n + 1], d_ids u64[total], d_valid u8[n], in buffers of the workspace that only locate requests
 * write: valid until the next locate request on it, untouched by edges / links requests. */
gbwt_hip_status gbwt_hip_locate_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const gbwt_hip_state *states, uint64_t n, int unique, gbwt_hip_located *out);
/* ... for states that are in HBM already -- the d_states of a gbwt_hip_search_device result: search -> locate without leaving the device.
 * d_valid (may be NULL): states with d_valid[k] == 0, the failed searches, are invalid as they are. */
gbwt_hip_status gbwt_hip_locate_states_device(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const gbwt_hip_state *d_states, const uint8_t *d_valid, uint64_t n,
                                              int unique, gbwt_hip_located *out);
gbwt_hip_status gbwt_hip_locate_positions(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const gbwt_hip_pos *positions, uint64_t n, uint64_t *ids, uint8_t *valid);
/* Device time (HIP events) of the last locate request for states on `ws`: the locate kernel; sort, flags, scan and compaction of a unique
 * request (0 otherwise). */
gbwt_hip_status gbwt_hip_last_locate_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *sort_ms);
/* The LF steps the lanes of a states request take: the same kernel launched once more with a counter, outside any timing.  *steps / *positions
 * = steps per located position. */
gbwt_hip_status gbwt_hip_locate_count_steps(const gbwt_hip_index *index, gbwt_hip_workspace *ws, const gbwt_hip_state *states, uint64_t n, uint64_t *steps,
                                            uint64_t *positions);
/* The locate index of a handle; all zeros before the first locate call has built it.  interval = GBWT_HIP_LOCATE_INTERVAL as read at open;
 * device_bytes = what the index adds to index_device_bytes; build_launches = kernels, scans and sorts of the build. */
typedef struct {
    uint32_t built, interval;
    uint64_t sampled_records, table_positions, end_entries, device_bytes;
    double build_ms;
    uint32_t build_launches, reserved;
} gbwt_hip_locate_info;
gbwt_hip_status gbwt_hip_locate_index_info(const gbwt_hip_index *index, gbwt_hip_locate_info *out);

/* ---- construction: an index from a set of paths ------------------------------------------------------------------------------------------
 * What the C++ GBWT's builder does and the reference lacks ("GBWT construction" leads the list of what its README leaves open): the GBWT of
 * a set of paths, made on the device.  The result is a handle like any other -- a bare GBWT: no metadata, no graph -- opened the way
 * gbwt_hip_open_records_flags opens one (`flags` as there).
 *
 * A path set is a CSR over GBWT-encoded nodes (2 * id + orientation, id >= 1, so every node is >= 2): path p = nodes[offsets[p] ..
 * offsets[p + 1]), offsets[0] = 0.  bidirectional != 0: sequence 2p is path p and sequence 2p + 1 its reverse with every node flipped
 * (support::reverse_path); bidirectional == 0: sequence p is path p.  Zero paths, and paths without nodes, are valid.
 *
 * The index: alphabet_offset = smallest node - 1 and alphabet_size = largest node + 1 over the SEQUENCES (0 and 1 when nobody visits a
 * node); record r is node r + alphabet_offset, record 0 the endmarker's, a node nobody visits the one byte 0.  A record lists the successor
 * (0 at the end of the sequence) of every visit of its node, the visits ordered by reverse prefix: the nodes before the visit read
 * backwards, node by node; the start of a sequence is below every node, two visits whose prefixes reach the start together are ordered by
 * sequence id.  The endmarker's record lists the first node of every sequence (0 for an empty one) in sequence order.  Edge v -> w carries
 * the number of visits of w whose predecessor is smaller than v (0 for w = 0 and in the endmarker's record).  Bytes as BWTBuilder::append
 * writes them (src/bwt.rs:241-253; ByteCode src/support.rs:1063-1070, RLE src/support.rs:1238-1248).
 *
 * Widths.  The construction counts in 32 bits: every node, the number of sequences, and visits + sequences (over the sequences, so twice
 * the paths' for a bidirectional index) must fit 32 bits -- at most 2^32 - 1 --, and the alphabet must hold fewer than 2^30 records; beyond that:
 * GBWT_HIP_UNSUPPORTED, as at an open.  GBWT_HIP_BAD_ARGUMENT, before the device is touched: a null pointer (nodes may be NULL when
 * offsets[n_paths] = 0, offsets when n_paths = 0 as well), bidirectional other than 0 / 1, bad flags, offsets that do not start at 0 or
 * that decrease, a node below 2.  The nodes of gbwt_hip_build_from_rows_device are checked on the device (same status).
 *
 * gbwt_hip_build_from_rows_device: the same for rows that lie in HBM of `device` already, in the layout gbwt_hip_extract_device leaves in a
 * gbwt_hip_paths: d_offsets u64[n_paths + 1], d_nodes u32.  The rows are only read; the call returns when the handle is open. */
gbwt_hip_status gbwt_hip_build_from_paths(const uint64_t *offsets, const uint64_t *nodes, uint64_t n_paths, int bidirectional, int device, uint32_t flags,
                                          gbwt_hip_index **out);
gbwt_hip_status gbwt_hip_build_from_rows_device(const uint64_t *d_offsets, const uint32_t *d_nodes, uint64_t n_paths, int bidirectional, int device, uint32_t flags,
                                                gbwt_hip_index **out);
/* The record stream and the dense record starts of any handle, from its host image: record r = data[starts[r] .. starts[r + 1]), the last
 * one ends at *data_len (the inputs of gbwt_hip_open_records).  *data_len and *n_records are always filled; the bytes are copied when
 * out_data != NULL and out_starts != NULL and both capacities suffice (else GBWT_HIP_CAPACITY; both NULL is a size query). */
gbwt_hip_status gbwt_hip_records(const gbwt_hip_index *index, uint8_t *out_data, uint64_t data_capacity, uint64_t *data_len, uint64_t *out_starts,
                                 uint64_t starts_capacity, uint64_t *n_records);
/* Writes the handle in the simple-sds format (Serialize for GBWT, src/gbwt.rs:389-400; for GBZ, src/gbz.rs:662-672): a GBZ handle as a
 * GBZ v1 container, a GBWT handle as a GBWT file.  A file that was loaded is written back as it was. */
gbwt_hip_status gbwt_hip_save(const gbwt_hip_index *index, const char *path);
/* The construction behind a handle; all zeros (built = 0) for a handle that was not built.  visits / sequences: over the sequences;
 * rounds: doubling rounds of the ranking, at most ceil(log2(longest sequence + 1)); peak_scratch_bytes: the most HBM the construction
 * held at once besides the caller's rows (all given back before the open); *_ms: HIP events around the four phases; open_ms: host
 * clock around the open behind them. */
typedef struct {
    uint64_t visits, sequences, records, data_bytes, peak_scratch_bytes;
    uint32_t rounds, built;
    float expand_ms, rank_ms, edges_ms, encode_ms;
    double open_ms;
} gbwt_hip_build_info;
gbwt_hip_status gbwt_hip_last_build_info(const gbwt_hip_index *index, gbwt_hip_build_info *out);

/* ---- construction from GFA: gbunzip's inverse ------------------------------------------------------------------------------------------------
 * A GFA file, or a GFA text in host memory, becomes a GBZ handle like any loaded one -- records, metadata, tags and node labels --, parsed
 * and built on the device.  The rows of the paths go from the parse to the construction above without leaving HBM; the index is
 * bidirectional and is exactly that construction over the rows.
 *
 * Accepted input.
 *   Lines end in '\n'; the last one may lack it; empty lines are skipped.  A '\r' anywhere: GBWT_HIP_INVALID_DATA.  A line whose first byte
 *   is not H, S, L, P or W is ignored (and counted).
 *   H: the value of an RS:Z: field (of the first H-line that has one) becomes the tag reference_samples of the GBWT and of the GBZ, verbatim.
 *   S <name> <sequence> [...]: name is a decimal node id in 1 .. 2^31 - 1 without sign or leading zero; sequence is one or more bytes
 *     ("*" is refused); later fields are ignored.  A name that is not such an integer: GBWT_HIP_UNSUPPORTED -- it needs a node-to-segment
 *     translation, which is not built.  A second S-line of an id: INVALID_DATA.  Nothing is chopped: a label has any length.
 *   L: at least five fields, and not otherwise read.  The edges of the result are those the paths use, as in a GBWTGraph: a link that no
 *     path crosses is not in the result, and gbwt_hip_write_gfa will not print it.
 *   P <name> <steps> [...]: steps = id+ / id- joined by ','; an empty field or "*" = no steps.  The name is NOT parsed as PanSN: every
 *     P-line is a generic path (sample _gbwt_ref, the whole name as contig, haplotype 0, fragment 0).
 *   W <sample> <hap> <contig> <start> <end> <walk>: walk = >id / <id; empty or "*" = no steps; hap a decimal number below 2^32 - 1; start
 *     a decimal number below 2^32, or "*" = 0; end is not read.  The path is (sample, contig, hap, start).
 *   Every step names a segment with an S-line anywhere in the file (else INVALID_DATA); line order is free.
 *   Path order: the P-lines in file order, then the W-lines in file order -- what gbunzip writes, so a file it wrote keeps its path ids.
 *   Metadata: sample names "_gbwt_ref" (iff there is a P-line), then the W samples by first appearance; contig names by first appearance
 *     over the paths in path order; haplotypes = distinct (sample, haplotype).  Two paths with the same four fields: INVALID_DATA.
 *   Graph: no translation; a segment that no path visits has no node in a GBZ, and its label is dropped.
 *   A refusal names the 1-based number of the FIRST offending line in file order, and nothing is constructed.  Sizes beyond the widths of
 *   the construction above: GBWT_HIP_UNSUPPORTED, in its wording; more than 2^31 - 1 lines likewise.
 * GBWT_HIP_BAD_ARGUMENT (null path / text with len > 0 / out, bad flags) and GBWT_HIP_IO_ERROR (a file that cannot be read) answer before
 * the device is touched.  `flags` as in gbwt_hip_open_file_flags. */
gbwt_hip_status gbwt_hip_build_from_gfa(const char *path, int device, uint32_t flags, gbwt_hip_index **out);
gbwt_hip_status gbwt_hip_build_from_gfa_text(const char *text, uint64_t len, int device, uint32_t flags, gbwt_hip_index **out);
/* The parse behind a handle made from GFA; all zeros for every other handle (gbwt_hip_last_build_info answers for the construction).
 * lines: the non-empty ones, of which headers + segments + links + p_lines + w_lines + ignored_lines; steps: of all paths; label_bytes:
 * the sequences of all S-lines; tile_bytes: the text a wave reads at once; peak_parse_bytes: the most HBM the parse held at once (text
 * and tables, without the rows; all given back before the construction starts); structure / steps / labels: HIP events around the three
 * phases; read / upload / metadata: host clock around the mapping of the file, the copy of the text to the device, and the metadata. */
typedef struct {
    uint64_t bytes, lines, headers, segments, links, p_lines, w_lines, ignored_lines, steps, label_bytes, tile_bytes, peak_parse_bytes;
    float structure_ms, steps_ms, labels_ms, reserved;
    double read_ms, upload_ms, metadata_ms;
} gbwt_hip_gfa_info;
gbwt_hip_status gbwt_hip_last_gfa_info(const gbwt_hip_index *index, gbwt_hip_gfa_info *out);
/* ---- construction from GFA with a node-to-segment translation: segment names of any kind, long segments chopped --------------------------------
 * The calls above with options.  opts == NULL or {0, GBWT_HIP_GFA_TRANSLATE_NEVER} IS the call above, byte for byte and message for message.
 * NEVER with max_node_length > 0, an unknown `translate` or a nonzero `reserved`: GBWT_HIP_BAD_ARGUMENT before the device is touched.
 * AUTO translates iff the name of an S-line (with its three fields) is not a node id under the rule above, or max_node_length > 0 and a
 * sequence is longer; over a text that needs neither it gives the handle NEVER gives (translated == 0).  A text without S-lines, or one
 * whose paths visit nothing, has no nodes and gets no translation under any option.
 *
 * A translated build (what gfa2gbwt --max-node makes; pinned by tests/golden/translation.gbz):
 *   Segments are ALL S-lines in file order.  Segment k with a sequence of L bytes owns max(1, ceil(L / max_node_length)) consecutive node
 *     ids (one if max_node_length == 0); the first segment starts at node 1.  The mapping has a one at the first node of every segment
 *     and its universe is the number of nodes + 1.  Every node but the last of its segment carries exactly max_node_length bytes.
 *   A segment that no path visits keeps its node range; its stored name is empty and its nodes have neither labels nor records.
 *   A name is any 1 .. 255 bytes without tab or newline.  An empty name: INVALID_DATA; a longer one: UNSUPPORTED; a second S-line of a
 *     name: INVALID_DATA on the LATER line.
 *   P steps are split at ','; a token is a name followed by one byte '+' or '-' (the name may hold those bytes).  A W walk is split at
 *     '>' and '<'.  An empty token, a token without its orientation, a trailing ',' or a walk that does not start with a mark:
 *     INVALID_DATA.  A name without an S-line: INVALID_DATA.  The empty field and "*" are no steps, as above.
 *   A forward step on segment k becomes its nodes ascending, each forward; a reverse step its nodes descending, each reverse.
 *   Path order, metadata, RS:Z:, L-lines, ignored lines and the rule of the first offending line are those above.  More than 2^31 - 1
 *     nodes: UNSUPPORTED; the visits counted against the widths of the construction are the NODES of the steps.
 *   The handle has stats.has_translation == 1 and the dense labels of a loaded translated GBZ (one per node 1 .. nodes);
 *   gbwt_hip_save writes the translation, and every segment or link query and gbwt_hip_write_gfa answer as for a loaded file.
 *   gbwt_hip_gfa_info.steps counts the steps of the text, gbwt_hip_build_info.visits the nodes they became (twice: bidirectional). */
#define GBWT_HIP_GFA_TRANSLATE_NEVER  0   /* the rules of gbwt_hip_build_from_gfa */
#define GBWT_HIP_GFA_TRANSLATE_AUTO   1   /* translate iff a name is not a node id under those rules, or a sequence is longer than max_node_length */
#define GBWT_HIP_GFA_TRANSLATE_ALWAYS 2
typedef struct {
    uint32_t max_node_length;   /* 0: never chop; gfa2gbwt's default is 1024 */
    uint32_t translate;
    uint64_t reserved[2];       /* must be 0 */
} gbwt_hip_gfa_options;
gbwt_hip_status gbwt_hip_build_from_gfa_opts(const char *path, const gbwt_hip_gfa_options *opts, int device, uint32_t flags, gbwt_hip_index **out);
gbwt_hip_status gbwt_hip_build_from_gfa_text_opts(const char *text, uint64_t len, const gbwt_hip_gfa_options *opts, int device, uint32_t flags, gbwt_hip_index **out);
/* The translation behind a handle made from GFA; all zeros for every other handle, and all but `segments` for an untranslated build.
 * nodes: all node ids, visited or not; chopped_segments: those with more than one node; name_bytes: the stored names (of the visited
 * segments); table_bytes: the name table in HBM (positions, lengths, sorted hashes, ranks, buckets); names_ms: hashing, sort, duplicate
 * check and buckets; expand_ms: steps to nodes.  Both are HIP events and lie inside gbwt_hip_gfa_info.steps_ms. */
typedef struct {
    uint64_t translated, segments, nodes, chopped_segments, unvisited_segments, name_bytes, table_bytes;
    float names_ms, expand_ms;
    float reserved[2];
} gbwt_hip_gfa_translation_info;
gbwt_hip_status gbwt_hip_last_gfa_translation_info(const gbwt_hip_index *index, gbwt_hip_gfa_translation_info *out);

/* The counts of a GFA file without a device and without the checks of a construction (only a '\r' is refused): bytes .. label_bytes and
 * tile_bytes are filled, steps = the orientation marks of the step fields. */
gbwt_hip_status gbwt_hip_parse_gfa(const char *path, gbwt_hip_gfa_info *out);

/* ---- merging: one index from two ---------------------------------------------------------------------------------------------------------
 * The index of the sequences of `a` in order, then the sequences of `b` in order: byte for byte what gbwt_hip_build_from_paths returns for
 * that input -- record stream, record starts, sequences, size, alphabet_offset, alphabet_size, bidirectional.  The inputs are taken as
 * SEQUENCES: in bidirectional inputs the pairs 2p / 2p + 1 stay as they are, path p of b becomes path paths(a) + p.  The result is opened
 * with `flags` as by gbwt_hip_open_records_flags; a and b are only read and stay usable.  The alphabet of the result is the union of the
 * alphabets the headers of the inputs state (an input without visits has none).
 *
 * GBWT_HIP_BAD_ARGUMENT, before the device is touched: a null a, b or out; bad flags; an unknown algorithm; a nonzero reserved field;
 * handles on different devices; one input bidirectional and the other not; one input a GBZ and the other a bare GBWT; _INSERT for
 * unidirectional inputs.  *out is cleared by a call that fails.  Widths: those of the construction over the merged set (visits +
 * sequences at most 2^32 - 1, fewer than 2^30 records), else GBWT_HIP_UNSUPPORTED in its wording.
 *
 * Algorithms.  INSERT (bidirectional inputs only): the input with fewer visits (b on a tie) is walked, one lane per
 * sequence, through itself and -- with the successor forced -- through the other input, which gives every visit its rank among the
 * other's; the record bodies of both are interleaved by those ranks and encoded by the construction's own phases.  Nothing is ranked or
 * sorted by prefix.  It reads the record bytes, the record starts and the endmarker of the inputs, which every handle keeps, whatever
 * it was opened for.  REBUILD: gbwt_hip_extract_device of all sequences of both (the inputs must be open for extraction), the rows
 * behind one another, and the construction over them.  AUTO: REBUILD where both inputs are open for extraction or unidirectional, else
 * INSERT.  (The walk of INSERT is one dependent chain per sequence of the smaller input; on 100 000 sites x 1 000 haplotypes REBUILD took
 * 0.66 s against 2.36 s for 500 + 500 haplotypes and 0.63 s against 1.72 s for 990 + 10: profiles/r16_merge_halves.json, _insert.json.)
 *
 * Metadata (assembled on the host).  Neither input has it: none.  Exactly one has it, or one lacks path, sample or contig names:
 * GBWT_HIP_UNSUPPORTED.  Else sample names are a's in order, then those of b that a lacks, in b's order; contig names likewise; path
 * names are a's, then b's with sample and contig ids remapped.  A path of b whose four fields equal those of an earlier path:
 * GBWT_HIP_INVALID_DATA, naming the path id in b.  haplotype_count = distinct (sample, phase) over the merged path names.  Tags of the
 * GBWT and of the GBZ: a's, then the keys only b has; reference_samples is a's names, then those of b's that are not among them, joined
 * by one space (absent when both lack it).  Document-array samples are dropped.
 * Graph (two GBZ): the union of the node labels; a node labelled differently in the two: GBWT_HIP_INVALID_DATA, naming the node; an
 * input with a node-to-segment translation: GBWT_HIP_UNSUPPORTED.  The result answers every call as a loaded file does. */
#define GBWT_HIP_MERGE_AUTO    0   /* rebuild where it can run (both inputs open for extraction, or unidirectional), else insertion */
#define GBWT_HIP_MERGE_REBUILD 1   /* extract both to rows in HBM, concatenate, run the construction */
#define GBWT_HIP_MERGE_INSERT  2   /* insertion, asked for by name */
typedef struct { uint32_t algorithm; uint32_t reserved32; uint64_t reserved[2]; } gbwt_hip_merge_options;   /* reserved: 0; NULL: AUTO */
gbwt_hip_status gbwt_hip_merge(const gbwt_hip_index *a, const gbwt_hip_index *b, const gbwt_hip_merge_options *opts,
                               uint32_t flags, gbwt_hip_index **out);
/* The merge behind a handle; all zeros for a handle that was not merged.  visits .. data_bytes: of the result; peak_scratch_bytes: the
 * most HBM the merge held at once (without the inputs); walked_input: 0 = a, 1 = b, with its sequences and visits (INSERT only);
 * algorithm_used: _INSERT or _REBUILD; rounds: the doubling rounds of a REBUILD; walk .. encode: HIP events around the phases (a REBUILD
 * fills edges and encode only); metadata / open: host clock. */
typedef struct {
    uint64_t visits, sequences, records, data_bytes, peak_scratch_bytes, walked_sequences, walked_steps;
    uint32_t algorithm_used, walked_input /* 0 = a, 1 = b */, merged, rounds;
    float walk_ms, decode_ms, interleave_ms, edges_ms, encode_ms;
    double metadata_ms, open_ms;
} gbwt_hip_merge_info;
gbwt_hip_status gbwt_hip_last_merge_info(const gbwt_hip_index *index, gbwt_hip_merge_info *out);

/* ---- removal: an index without some of its paths ------------------------------------------------------------------------------------------
 * The index of the sequences of `index` that do not belong to the paths path_ids[0, n), in their old order and renumbered densely: byte
 * for byte what gbwt_hip_build_from_paths returns for those sequences -- record stream, record starts, sequences, size, alphabet_offset,
 * alphabet_size, bidirectional.  In a bidirectional index path p is the sequences 2p and 2p + 1, in a unidirectional one sequence p.
 * alphabet_offset and alphabet_size are those of the kept sequences, as the construction defines them: the alphabet shrinks when the
 * smallest or the largest visited node goes, and a node that nobody visits any more has the record of one byte 0.  n == 0 gives a copy
 * built from all sequences; removing every path gives the index of a set without sequences.  The result is opened with `flags` as by
 * gbwt_hip_open_records_flags; the input is only read and stays usable.
 *
 * GBWT_HIP_BAD_ARGUMENT, before the device is touched: a null index or out; null path_ids with n > 0; bad flags; an unknown algorithm; a
 * nonzero reserved field; a path id at or above the number of paths, or one that appears twice (the message names the id); _REBUILD on
 * a handle that is not open for extraction.  *out is cleared by a call that fails.
 * Widths: those of the construction (visits + sequences at most 2^32 - 1), else GBWT_HIP_UNSUPPORTED in its wording -- for DELETE over
 * the INPUT, whose positions it lays out, and before the device is touched; for REBUILD over the kept sequences, before the device is
 * touched where the input is within the widths or the kept sequences alone are beyond them, else behind the extraction and before the
 * construction.  A larger index loses paths by REBUILD when what is kept fits.
 *
 * Algorithms.  DELETE (bidirectional or not): all positions of all records form one array; one lane per removed sequence
 * follows it with the plain LF step and marks its positions, a prefix sum over the marks moves every kept position forward, and the
 * compacted record bodies are encoded by the construction's own phases.  The offset of a kept edge v -> w is its old offset P less the
 * marks among the first P positions of w's old record.  Nothing is ranked or sorted by prefix, and no atomics are used.  It reads the
 * record bytes, the record starts and the endmarker, which every handle keeps, whatever it was opened for.  REBUILD:
 * gbwt_hip_extract_device of the kept sequences and the construction over those rows.  AUTO: REBUILD where the handle is open for
 * extraction, else DELETE -- the rule of gbwt_hip_merge, which the measurement confirmed.  (The walk of DELETE is one dependent chain per
 * removed sequence; on 100 000 sites x 1 000 haplotypes DELETE took 1 245 ms against 630 ms of REBUILD for 10 removed haplotypes and
 * 1 348 ms against 301 ms for 500: profiles/r17_remove_few.json, _half.json, tools/remove_bench.py.)
 *
 * Metadata (assembled on the host).  None in the input: none.  Metadata without path, sample or contig names: GBWT_HIP_UNSUPPORTED.
 * Else the names of the removed paths go, and so do the sample names and the contig names that no kept path uses; the rest keep their
 * order and the ids in the kept path names are remapped.  haplotype_count = distinct (sample, phase) over the kept path names.  Tags of
 * the GBWT and of the GBZ are copied; reference_samples loses the names that were samples and no longer are, and is absent when none is
 * left.  Document-array samples are dropped.
 * Graph (a GBZ): the labels of the nodes that are still visited, as in a construction from GFA.  A graph with a node-to-segment
 * translation: GBWT_HIP_UNSUPPORTED. */
#define GBWT_HIP_REMOVE_AUTO    0   /* rebuild where the handle is open for extraction, else deletion */
#define GBWT_HIP_REMOVE_REBUILD 1   /* extract the kept sequences to rows in HBM, run the construction */
#define GBWT_HIP_REMOVE_DELETE  2   /* mark, compact, re-encode; ranks nothing */
typedef struct { uint32_t algorithm; uint32_t reserved32; uint64_t reserved[2]; } gbwt_hip_remove_options;   /* reserved: 0; NULL: AUTO */
gbwt_hip_status gbwt_hip_remove_paths(const gbwt_hip_index *index, const uint64_t *path_ids, uint64_t n, const gbwt_hip_remove_options *opts,
                                      uint32_t flags, gbwt_hip_index **out);
/* The removal behind a handle; all zeros for a handle that did not come from one.  visits .. data_bytes: of the result;
 * peak_scratch_bytes: the most HBM the removal held at once (without the input); removed_sequences / removed_steps: the sequences that
 * went and their visits; algorithm_used: _DELETE or _REBUILD; rounds: the doubling rounds of a REBUILD; decode .. encode: HIP events around
 * the phases (a REBUILD fills edges and encode only) -- decode: lengths, scan and bodies; walk: the clearing of the marks, the copy of the
 * sequence ids to the device and the marking walk; compact: the prefix sum, the copy of its total to the host, the scatter and the
 * min / max reduction of the new alphabet; edges and encode: as in gbwt_hip_build_info; metadata / open: host clock. */
typedef struct {
    uint64_t visits, sequences, records, data_bytes, peak_scratch_bytes, removed_sequences, removed_steps;
    uint32_t algorithm_used, removed, rounds, reserved32;
    float walk_ms, decode_ms, compact_ms, edges_ms, encode_ms;
    double metadata_ms, open_ms;
} gbwt_hip_remove_info;
gbwt_hip_status gbwt_hip_last_remove_info(const gbwt_hip_index *index, gbwt_hip_remove_info *out);

/* ---- multi-GPU: the one exchange of a sharded extraction -------------------------------------------------------------
 * The reference's parallel axis is the path: rayon workers pull path ids and hand their finished lines to ONE writer behind a mutex
 * (src/bin/gbunzip.rs:27, 421-434).  Sharded over GPUs -- one process per GPU, the index replicated, path p on rank p mod world
 * (interleaved) or in contiguous blocks, no collective inside the walk -- that writer becomes an ordered gather on one rank, over RCCL:
 * an all-gather of the per-rank counts, ONE group of point-to-point sends (every peer streams to the root over its own xGMI link at
 * once), and kernels on the root that put the rows into path order.
 *
 * gbwt_hip_comm_unique_id: called by one rank; the 128 bytes travel to the others by whatever channel the host program has (a file,
 * a socket, MPI, a torch store).  gbwt_hip_comm_create: collective over the `world` ranks (ncclCommInitRank), each with its device.
 * RCCL is loaded at run time; without it these calls return GBWT_HIP_UNSUPPORTED and everything else works. */
typedef struct { char bytes[128]; } gbwt_hip_unique_id;
typedef struct gbwt_hip_comm gbwt_hip_comm;
gbwt_hip_status gbwt_hip_comm_unique_id(gbwt_hip_unique_id *out);
gbwt_hip_status gbwt_hip_comm_create(const gbwt_hip_unique_id *id, int rank, int world, int device, gbwt_hip_comm **out);
void gbwt_hip_comm_destroy(gbwt_hip_comm *comm);
/* gbwt_hip_gather_rows: the rows of the last gbwt_hip_extract_device on `ws` of EVERY rank (collective), gathered on `root` in path
 * order.  `interleaved` is the layout of the shards: GBWT_HIP_GATHER_BLOCKS = the rows of rank 0, then of rank 1, ...;
 * GBWT_HIP_GATHER_INTERLEAVED = row k of rank r is global row k * world + r (the ranks' row counts must be those of p -> rank p mod
 * world); GBWT_HIP_GATHER_PARTS = every rank holds its part of every row (gbwt_hip_extract_part_device with part = rank, parts = world,
 * the same ids everywhere): row k of the result is the parts of row k in rank order.  On the root *out describes the result -- device
 * memory of the communicator, valid until its next gather: d_offsets[rows + 1], d_nodes[total] --, elsewhere it is zeroed.
 * gbwt_hip_gather_lines: the same for the GFA lines of the last gbwt_hip_path_lines_device on `ws` (d_text, d_line_offsets): the final
 * GFA concatenation of north_star. */
enum { GBWT_HIP_GATHER_BLOCKS = 0, GBWT_HIP_GATHER_INTERLEAVED = 1, GBWT_HIP_GATHER_PARTS = 2 };
gbwt_hip_status gbwt_hip_gather_rows(gbwt_hip_comm *comm, const gbwt_hip_index *index, gbwt_hip_workspace *ws, int root, int interleaved,
                                     gbwt_hip_paths *out);
gbwt_hip_status gbwt_hip_gather_lines(gbwt_hip_comm *comm, const gbwt_hip_index *index, gbwt_hip_workspace *ws, int root, int interleaved,
                                      gbwt_hip_lines *out);
/* The last gather on `comm`, as this rank saw it: wall time from the first collective to the last kernel, bytes sent (peers) or
 * gathered (root), and whether the payload was staged through an ordinary allocation before the send (rows mapped from spread chunks;
 * GBWT_HIP_COMM_DIRECT=1 sends from the mapping). */
typedef struct { double ms; uint64_t bytes; uint32_t staged_send, reserved; } gbwt_hip_comm_stats;
gbwt_hip_status gbwt_hip_comm_last(const gbwt_hip_comm *comm, gbwt_hip_comm_stats *out);

/* ---- checking hooks for device-resident results -------------------------------------------------
 * Per-path sums of the node ids of the last gbwt_hip_extract_device call on `ws` (a wave-per-path
 * reduction on the device), copied to out_sums[n]: a cheap full-size checksum of the extraction. */
gbwt_hip_status gbwt_hip_path_sums(const gbwt_hip_index *index, gbwt_hip_workspace *ws, uint64_t *out_sums, uint64_t n);
/* The same with a checksum that depends on the ORDER of the nodes: out_hashes[k] = sum over the positions i of row k of
 * (node_i + 1) * splitmix64(i)  (mod 2^64; splitmix64(i): z = i + 0x9E3779B97F4A7C15, z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9,
 * z = (z ^ z >> 27) * 0x94D049BB133111EB, z ^ z >> 31).  What bench.py compares with the CPU oracle's walk of the same paths
 * (SequenceIter, src/gbwt.rs:557-568) at full size, where copying 13 GB of rows out to compare them would dominate the run. */
gbwt_hip_status gbwt_hip_path_hashes(const gbwt_hip_index *index, gbwt_hip_workspace *ws, uint64_t *out_hashes, uint64_t n);
/* Copies row k of the last device-resident extraction to host: out_nodes[min(len, capacity)], *len = row length. */
gbwt_hip_status gbwt_hip_copy_path(const gbwt_hip_index *index, gbwt_hip_workspace *ws, uint64_t k, uint32_t *out_nodes,
                                   uint64_t capacity, uint64_t *len);

/* ---- measurement hooks -------------------------------------------------------------------------
 * From HIP events on the workspace stream, for the last gbwt_hip_extract_device call: *walk_ms = duration of its
 * dominant kernel (the walk; bench.py's roofline object), *total_ms = everything the call put on the stream, from the
 * upload of the ids to the last kernel (lengths, offsets, walker order, walk; host waits in between included). */
gbwt_hip_status gbwt_hip_last_kernel_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *total_ms);
/* The same for the last GFA lines request (gbwt_hip_path_lines / _device) on `ws`: *walk_ms = the walk kernel of its extraction,
 * *format_ms = everything behind the walk on the stream -- sizes, scans, the one host wait for the total, the formatting kernel. */
gbwt_hip_status gbwt_hip_last_lines_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *format_ms);
/* Free and total memory of a device in bytes (hipMemGetInfo): what the tests use to see that a workspace gives its rows back. */
gbwt_hip_status gbwt_hip_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);
/* Kernel time (ms, HIP events on the workspace stream, host staging excluded) of the last navigation / search call
 * (start, forward, backward, find, extend, bd_*, search, bd_search and the *_device forms) on `ws`.  (With GBWT_HIP_QUERY_PIPELINE=1 a large
 * host-pointer call moves in chunks through the copy lanes and this is the span of the whole pipeline on the device, copies included.) */
gbwt_hip_status gbwt_hip_last_query_ms(const gbwt_hip_workspace *ws, float *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif
