#!/usr/bin/env python3
"""The graph of a config-4-shaped GBZ through the device: edge rows of every node and the H-, S- and L-lines of its GFA file, on one GPU,
next to the host preamble of gbwt_hip_write_gfa on the same index (the yardstick for a later decision about that preamble).

Synth.genome with labels of realistic length at the shape of tools/c4_bench.py's SIZES[size], as tools/sequences_bench.py builds it, but
without paths of the generic sample: write_gfa(path, PATHS_REF_ONLY) then writes the graph lines and nothing else.  One JSON line, also
written to profiles/r11_graph_<size>.json:

  nodes / edges_listed          nodes that exist; edges of all (node, orientation) rows, successors
  s_lines / l_lines / *_bytes   line counts and bytes of the device text (header_bytes apart)
  size_ms / segments_ms / links_ms   gbwt_hip_last_graph_ms: the first request (which sizes) and the best of the later ones (which only format)
  lines_per_s / text_bytes_per_s     over segments_ms + links_ms of the best formatting request
  edges_per_s                   edges_device over all nodes in both orientations: edges listed / kernel time (gbwt_hip_last_query_ms), best pass
  counted_bytes_per_line        ALGORITHMIC bytes, not measured traffic: an S-line = its text written + its label read + 8 B line offset +
                                8 B item; an L-line = its text written + 8 B edge + 4 B row + 16 B line offsets
  host_preamble_ms              wall time of write_gfa(PATHS_REF_ONLY) into tmpfs: median of the runs, and min / max (the spread)
  parity                        device text == the file the host preamble wrote
No speed-up is asserted."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def run(size="small", passes=3, host_runs=3, device=0):
    import c4_bench as C4
    import gbwt_rs_amd as G
    from gbwt_rs_amd import synth as S
    import bench
    p = dict(C4.SIZES[size])
    tmpdir = tempfile.mkdtemp(prefix="gbwt_graph_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        path = os.path.join(tmpdir, "c4.gbz")
        t0 = time.perf_counter()
        g = S.Synth.genome(contigs=p["contigs"], fragments=p["fragments"], haplotypes=p["haplotypes"], sites=p["sites"], seed=42, labels=1,
                           min_walkers=p["min_walkers"], wrap_contig=p["wrap_contig"], threads=min(16, os.cpu_count() or 1), generic_per_contig=0)
        g.save(path, as_gbz=True)
        gen_s = time.perf_counter() - t0
        gbz = G.GBZ.load(path, device=device, flags=G.OPEN_EXTRACT | G.OPEN_GFA)
        # edge rows of every node, both orientations
        nodes = gbz.node_iter()
        ids = np.repeat(nodes, 2)
        orient = np.tile(np.array([0, 1], dtype=np.uint8), nodes.size)
        edge_ms, edges = [], 0
        for k in range(passes + 1):
            gbz.edges_device(ids[:1], orient[:1])                  # (untimed) a request that repeats the last one would only find it there
            rows = gbz.edges_device(ids, orient)
            edges = int(rows.total)
            if k:                                                  # (the first pass sizes the workspace)
                edge_ms.append(gbz.last_query_ms())
        # graph lines: the first request sizes, the later ones format
        t0 = time.perf_counter()
        text = gbz.graph_lines_device()
        first_wall_ms = (time.perf_counter() - t0) * 1e3
        first = gbz.last_graph_ms()
        later = []
        for _ in range(passes):
            gbz.graph_lines_device()
            later.append(gbz.last_graph_ms())
        best = min(later, key=lambda t: t[1] + t[2])
        fmt_s = (best[1] + best[2]) * 1e-3
        # the host preamble on the same index
        out = os.path.join(tmpdir, "graph.gfa")
        host_ms = []
        for _ in range(max(3, host_runs)):
            t0 = time.perf_counter()
            gbz.write_gfa(out, G.PATHS_REF_ONLY)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        total = text.header_bytes + text.segment_bytes + text.link_bytes
        parity = os.path.getsize(out) == total
        if parity:
            got = gbz.graph_lines()
            with open(out, "rb") as f:
                parity = f.read() == got
        digits = np.searchsorted(10 ** np.arange(1, 20, dtype=np.uint64), nodes, side="right") + 1
        label_bytes = int(text.segment_bytes) - int((4 + digits).sum())
        counted_s = (text.segment_bytes + label_bytes + 16 * text.segments) / max(1, text.segments)
        counted_l = (text.link_bytes + 28 * text.links) / max(1, text.links)
        return {
            "tool": "graph_bench", "size": size, "workload": f"Synth.genome[{size} shape, labels 1..1024 bp, no generic paths, seed 42]",
            "nodes": int(nodes.size), "edges_listed": edges, "s_lines": int(text.segments), "l_lines": int(text.links), "header_bytes": int(text.header_bytes),
            "s_bytes": int(text.segment_bytes), "l_bytes": int(text.link_bytes), "generator_seconds": round(gen_s, 1),
            "first_request_wall_ms": round(first_wall_ms, 2), "first_request_ms": {"size": round(first[0], 3), "segments": round(first[1], 3), "links": round(first[2], 3)},
            "format_ms": {"segments": round(best[1], 3), "links": round(best[2], 3)}, "passes": passes,
            "lines_per_s": (text.segments + text.links) / fmt_s, "text_bytes_per_s": (text.segment_bytes + text.link_bytes) / fmt_s,
            "edges_kernel_ms": [round(x, 3) for x in edge_ms], "edges_per_s": edges / (min(edge_ms) * 1e-3),
            "counted_bytes_per_s_line": round(counted_s, 2), "counted_bytes_per_l_line": round(counted_l, 2), "counted_bytes_are": "algorithmic",
            "host_preamble_ms": {"median": round(statistics.median(host_ms), 2), "min": round(min(host_ms), 2), "max": round(max(host_ms), 2), "runs": len(host_ms)},
            "parity_ok": bool(parity), "source_fingerprint": bench.source_fingerprint(),
        }
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="small", choices=["tiny", "medium", "small", "full"])
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--host-runs", type=int, default=3, help="runs of the host preamble (three at least)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="", help="the JSON file (default: profiles/r11_graph_<size>.json)")
    a = ap.parse_args()
    res = run(a.size, a.passes, a.host_runs, a.device)
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", f"r11_graph_{a.size}.json"), "w") as f:
        f.write(line + "\n")
    return 0 if res["parity_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
