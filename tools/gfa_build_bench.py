#!/usr/bin/env python3
"""Construction from GFA on the device (include/gbwt_hip.h, "construction from GFA") on one GPU: the GFA text of a config-4-shaped GBZ back
into a GBZ.

Synth.genome at the shape of tools/c4_bench.py's SIZES[size] with labels of realistic length is saved, loaded and written with write_gfa --
all outside the timed part.  GBZ.from_gfa then runs behind a warm-up build of a small text, --passes times.  The records of the last build
are compared with GBWT.from_paths over the rows of the index the GFA came from, re-ordered to the GFA's path order (the generic paths,
then the others).  One JSON line, also written to profiles/r14_gfa_build_<size>.json; times are medians over the passes, *_all the spread:

  structure_ms / steps_ms / labels_ms   HIP events around the three phases of the parse;  parse_ms their sum
  build_ms                      the four phases of the construction behind it;  open_ms: the open;  wall_ms: host clock around the call
  read_ms / upload_ms / metadata_ms     host clock: mapping the file, text to the device, metadata from the name fields
  text_gb_per_s                 text bytes over every parse phase, over parse_ms, and over parse_ms + build_ms
  counted                       ALGORITHMIC bytes per phase, not measured traffic, per text byte and -- over the phase's time -- as a share of
                                8 TB/s.  structure: the text twice + 8 B per line (newline positions; the tab positions are not counted) +
                                41 B per line written and 41 B read again (line tables); steps: the text twice + 4 B per step + 32 B per
                                tile; labels: the kept label bytes read and written + 8 B per S-line
  peak_parse_bytes              the most HBM the parse held at once (text and tables, without the rows)
A phase far below the share of the others at the same bytes is bound by issue, not by bandwidth.  No speed-up and no threshold is stated.

--translate (with --max-node N, default 1024: gfa2gbwt's) builds the SAME text once more with a node-to-segment translation
(GFA_TRANSLATE_ALWAYS) and reports, under "translated", its phase times next to the untranslated ones, names_ms and expand_ms (inside
steps_ms), the bytes of the name table per segment, and counted bytes per text byte of the two new phases -- names: name bytes read + 24 B
per segment written, sorted (24 B read and written) and read again + 4 B per bucket; expand: 12 B per step + 4 B per node.  The text has
integer names in ascending order, every segment on a path and labels no longer than N, so the translated build is the untranslated one
with the node ids renumbered 1 .. n: its records must be those of GBWT.from_paths over the source's rows renumbered that way
(records_equal, and the exit status), and the records of the untranslated build themselves where the ids have no gaps (ids_dense).  The
line then goes to profiles/r15_gfa_translate_<size>.json."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_BYTES_PER_S = 8e12


def translated_passes(G, gfa_path, passes, device, max_node, rows, plain_records, plain_phases, text_bytes):
    """The translated build of the same text: times, table and counted bytes, and whether its records are those of the source's rows with
    the node ids renumbered by rank."""
    infos, trs, dev = [], [], None
    for _ in range(passes):
        if dev is not None:
            dev.close()
        dev = G.GBZ.from_gfa(gfa_path, device=device, max_node=max_node, translate=G.GFA_TRANSLATE_ALWAYS)
        infos.append(dev.last_gfa_info())
        trs.append(dev.last_gfa_translation_info())
    data, starts = dev.records()
    header = (dev.sequences(), dev.len(), dev.alphabet_offset(), dev.alphabet_size())
    dev.close()
    ids = np.unique(np.concatenate([np.asarray(r, dtype=np.uint64) >> np.uint64(1) for r in rows])) if rows else np.zeros(0, dtype=np.uint64)
    dense = [((np.searchsorted(ids, np.asarray(r, dtype=np.uint64) >> np.uint64(1)).astype(np.uint64) + np.uint64(1)) << np.uint64(1)) | (np.asarray(r, dtype=np.uint64) & np.uint64(1)) for r in rows]
    witness = G.GBWT.from_paths(dense, bidirectional=True, device=device)
    w_data, w_starts = witness.records()
    equal = bytes(data) == bytes(w_data) and np.array_equal(starts, w_starts) and header == (witness.sequences(), witness.len(), witness.alphabet_offset(), witness.alphabet_size())
    witness.close()
    ids_dense = bool(len(ids) and int(ids[0]) == 1 and int(ids[-1]) == len(ids))
    if ids_dense:
        equal = equal and bytes(data) == plain_records[0] and np.array_equal(starts, plain_records[1]) and header == plain_records[2]
    med = lambda rows_, key: float(np.median([r[key] for r in rows_]))
    tr, info = trs[-1], infos[-1]
    phases = {k: med(infos, k) for k in ("structure_ms", "steps_ms", "labels_ms")}
    sub = {k: med(trs, k) for k in ("names_ms", "expand_ms")}
    segments = max(1, tr["segments"])
    buckets = 1 + (1 << max(0, int(segments - 1).bit_length()))
    counted = {"names_ms": tr["name_bytes"] + 24 * segments * 4 + 4 * buckets, "expand_ms": 12 * info["steps"] + 4 * tr["nodes"]}
    return {
        "max_node": max_node, **{k: int(tr[k]) for k in ("translated", "segments", "nodes", "chopped_segments", "unvisited_segments", "name_bytes", "table_bytes")},
        **phases, **sub, "parse_ms": sum(phases.values()), "untranslated": plain_phases,
        "table_bytes_per_segment": tr["table_bytes"] / segments, "peak_parse_bytes": int(info["peak_parse_bytes"]), "peak_parse_bytes_per_text_byte": info["peak_parse_bytes"] / text_bytes,
        "counted": {k[:-3]: {"bytes_per_text_byte": counted[k] / text_bytes, "share_of_8_tb_per_s": counted[k] / (sub[k] * 1e-3) / HBM_BYTES_PER_S if sub[k] else 0.0} for k in sub},
        "records_equal": bool(equal), "ids_dense": ids_dense,
    }


def run(size="small", passes=3, device=0, translate=False, max_node=1024):
    import bench
    import c4_bench as C4
    import gbwt_rs_amd as G
    from gbwt_rs_amd import synth as S
    p = dict(C4.SIZES[size])
    tmpdir = tempfile.mkdtemp(prefix="gbwt_gfa_build_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        gbz_path, gfa_path = os.path.join(tmpdir, "c4.gbz"), os.path.join(tmpdir, "c4.gfa")
        g = S.Synth.genome(contigs=p["contigs"], fragments=p["fragments"], haplotypes=p["haplotypes"], sites=p["sites"], seed=42, labels=1,
                           min_walkers=p["min_walkers"], wrap_contig=p["wrap_contig"], threads=min(16, os.cpu_count() or 1))
        g.save(gbz_path, as_gbz=True)
        generic = set(int(x) for x in g.generic_paths())
        n_paths = g.paths
        del g
        source = G.GBZ.load(gbz_path, device=device)
        source.write_gfa(gfa_path)
        order = np.array(sorted(generic) + [k for k in range(n_paths) if k not in generic], dtype=np.uint64)
        offsets, nodes = source.paths_csr(order)
        rows = [nodes[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]
        source.close()
        G.GBZ.from_gfa_text(b"S\t1\tA\nS\t2\tC\nP\tp\t1+,2-\nW\ts\t1\tc\t0\t2\t>1>2\n", device=device).close()      # warm-up: the runtime, the kernels
        infos, builds, wall, dev = [], [], [], None
        for _ in range(passes):
            if dev is not None:
                dev.close()
            t0 = time.perf_counter()
            dev = G.GBZ.from_gfa(gfa_path, device=device)
            wall.append((time.perf_counter() - t0) * 1e3)
            infos.append(dev.last_gfa_info())
            builds.append(dev.last_build_info())
        data, starts = dev.records()
        header = (dev.sequences(), dev.len(), dev.alphabet_offset(), dev.alphabet_size())
        dev.close()
        plain_records = (bytes(data), np.array(starts), header)
        witness = G.GBWT.from_paths(rows, bidirectional=True, device=device)
        w_data, w_starts = witness.records()
        parity = bytes(data) == bytes(w_data) and np.array_equal(starts, w_starts) and header == (witness.sequences(), witness.len(), witness.alphabet_offset(), witness.alphabet_size())
        witness.close()
        info = infos[-1]
        med = lambda rows_, key: float(np.median([r[key] for r in rows_]))
        phases = {k: med(infos, k) for k in ("structure_ms", "steps_ms", "labels_ms")}
        parse_ms = sum(phases.values())
        build_ms = sum(med(builds, k) for k in ("expand_ms", "rank_ms", "edges_ms", "encode_ms"))
        text_bytes, lines, steps, tiles = info["bytes"], info["lines"], info["steps"], -(-info["bytes"] // info["tile_bytes"])
        counted = {"structure_ms": 2 * text_bytes + (8 + 82) * lines, "steps_ms": 2 * text_bytes + 4 * steps + 32 * tiles,
                   "labels_ms": 2 * info["label_bytes"] + 8 * info["segments"]}
        gbs = lambda ms: text_bytes / (ms * 1e-3) / 1e9 if ms else 0.0
        translated = translated_passes(G, gfa_path, passes, device, max_node, rows, plain_records, dict(phases), text_bytes) if translate else None
        return {
            **({"translated": translated} if translate else {}),
            "tool": "gfa_build_bench", "size": size, "workload": f"GFA of Synth.genome {p}", "passes": passes,
            **{k: int(info[k]) for k in ("bytes", "lines", "segments", "links", "p_lines", "w_lines", "ignored_lines", "steps", "label_bytes", "tile_bytes", "peak_parse_bytes")},
            **phases, "parse_ms": parse_ms, "build_ms": build_ms, "open_ms": med(builds, "open_ms"), "wall_ms": float(np.median(wall)),
            "read_ms": med(infos, "read_ms"), "upload_ms": med(infos, "upload_ms"), "metadata_ms": med(infos, "metadata_ms"),
            "text_gb_per_s": {**{k[:-3]: gbs(v) for k, v in phases.items()}, "parse": gbs(parse_ms), "parse_and_build": gbs(parse_ms + build_ms)},
            "counted": {k[:-3]: {"bytes_per_text_byte": counted[k] / text_bytes, "share_of_8_tb_per_s": counted[k] / (phases[k] * 1e-3) / HBM_BYTES_PER_S if phases[k] else 0.0}
                        for k in phases},
            "peak_parse_bytes_per_text_byte": info["peak_parse_bytes"] / text_bytes,
            "parse_ms_all": [round(i["structure_ms"] + i["steps_ms"] + i["labels_ms"], 3) for i in infos], "wall_ms_all": [round(w, 1) for w in wall],
            "parity_ok": bool(parity), "source_fingerprint": bench.source_fingerprint(),
        }
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", choices=["tiny", "medium", "small", "full"], default="small")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--translate", action="store_true", help="also build the same text with a node-to-segment translation and compare")
    ap.add_argument("--max-node", type=int, default=1024, help="with --translate: segments longer than this are chopped")
    ap.add_argument("--out", default="", help="where the JSON line goes (default: profiles/r14_gfa_build_<size>.json, with --translate r15_gfa_translate_<size>.json)")
    a = ap.parse_args()
    res = run(a.size, a.passes, a.device, a.translate, a.max_node)
    line = json.dumps(res)
    print(line, flush=True)
    default = f"r15_gfa_translate_{a.size}.json" if a.translate else f"r14_gfa_build_{a.size}.json"
    with open(a.out or os.path.join(ROOT, "profiles", default), "w") as f:
        f.write(line + "\n")
    return 0 if res["parity_ok"] and (not a.translate or res["translated"]["records_equal"]) else 1


if __name__ == "__main__":
    sys.exit(main())
