#!/usr/bin/env python3
"""GBZ::reference_positions (src/gbz.rs:600-657) over the reference paths of a config-4-shaped GBZ on one GPU.

Synth.genome at the shape of tools/c4_bench.py's SIZES[size], with labels of realistic length (1 .. 1 024 bp) whatever the size says; the
reference paths are its generic paths plus those of two samples named by a `reference_samples` tag.  One JSON line, also written to
profiles/r10_refpos_<size>.json:

  paths / nodes / kept        reference paths, the nodes on them (LF steps of the reference's loop), positions kept at --interval
  walk_ms                     the unchanged k_walk_direct extraction of the rows (HIP events)
  select_ms                   label lengths, two scans, successors, the pointer-doubling rounds, up to the host's wait for the total
  offsets_ms                  the LF walk that carries the in-record offsets and writes the positions
  nodes_per_s                 nodes / (walk + select + offsets); best of --passes requests, the first (which uploads the labels) apart
  rounds / launches           pointer-doubling rounds that marked something; kernels and scans behind the extraction
  scratch_bytes               what the workspace holds more once the request is made (24 B per node + the results), and per node
  parity                      a seeded sample of the reference paths against the reference's loop over the oracle's start / forward
  cpu_*                       the oracle's multi-threaded plain walk of the same sequences (no label lengths, no positions kept): a LOWER
                              BOUND on the reference's cost, which also calls sequence_len per step and runs on one thread
"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(size="small", interval=1000, passes=5, sample=4, device=0, cpu_threads=16):
    import c4_bench as C4
    import gbwt_rs_amd as G
    from gbwt_rs_amd import synth as S
    import bench
    import oracle_lib as O
    import refpos_expect as R
    p = dict(C4.SIZES[size])
    tmpdir = tempfile.mkdtemp(prefix="gbwt_refpos_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        path = os.path.join(tmpdir, "c4.gbz")
        t0 = time.perf_counter()
        g = S.Synth.genome(contigs=p["contigs"], fragments=p["fragments"], haplotypes=p["haplotypes"], sites=p["sites"], seed=42, labels=1,
                           min_walkers=p["min_walkers"], wrap_contig=p["wrap_contig"], threads=min(16, os.cpu_count() or 1))
        tag = "s0 s1"
        g.set_tag("reference_samples", tag)
        g.save(path, as_gbz=True)
        gen_s = time.perf_counter() - t0
        want_ids = R.reference_paths(g.sample_names, [int(x[0]) for x in g.path_names], tag)
        t0 = time.perf_counter()
        gbz = G.GBZ.load(path, device=device, flags=G.OPEN_EXTRACT | G.OPEN_GFA)
        open_ms = (time.perf_counter() - t0) * 1e3
        ids = gbz.reference_paths()
        ids_ok = ids.tolist() == want_ids
        mem0 = gbz.memory_usage()["workspace_device_bytes"]
        t0 = time.perf_counter()
        gbz.path_positions_device(ids, interval + 1)                          # (apart: the node labels reach HBM with the first request)
        first_wall_ms = (time.perf_counter() - t0) * 1e3
        best, wall_ms = None, []
        for k in range(passes):
            t0 = time.perf_counter()
            _, _, kept = gbz.path_positions_device(ids, interval + (k & 1))   # (another interval every time: nothing is answered from the memo)
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            times = gbz.last_positions_ms()
            if (k & 1) == 0 and (best is None or sum(times) < sum(best[0])):
                best = (times, kept, gbz.last_positions_rounds())
        (walk_ms, select_ms, offsets_ms), kept, (rounds, launches) = best
        scratch = gbz.memory_usage()["workspace_device_bytes"] - mem0
        rows = gbz.path_positions(ids, interval)
        nodes = int(sum(len(g.path(int(q))) for q in ids))
        # parity on a seeded sample of the paths
        oracle = O.OracleGBZ(path)
        gbwt = oracle.gbwt()
        lengths = {}
        rng = np.random.default_rng(7)
        picks = sorted(rng.choice(len(rows), size=min(sample, len(rows)), replace=False).tolist()) if rows else []
        parity = True
        for k in picks:
            pid = rows[k][0]
            for v in g.path(pid).tolist():
                if v >> 1 not in lengths:
                    lengths[v >> 1] = len(gbz.node_sequence(v >> 1))
            parity &= R.same([rows[k]], [R.positions_of(R.node_starts(gbwt, pid, lengths), pid, interval)])
        seq_ids = 2 * np.asarray(ids, dtype=np.uint64)
        t0 = time.perf_counter()
        steps = gbwt.extract_timed(seq_ids, cpu_threads)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        total_ms = walk_ms + select_ms + offsets_ms
        return {
            "tool": "refpos_bench", "size": size, "workload": f"Synth.genome[{size} shape, labels 1..1024 bp, seed 42], reference_samples = '{tag}' + generic: {len(ids)} paths, {nodes} nodes",
            "interval": interval, "paths": int(len(ids)), "nodes": nodes, "kept": int(kept), "bases": int(sum(r[1] for r in rows)),
            "longest_path_nodes": int(max((len(g.path(int(q))) for q in ids), default=0)),
            "open_ms": round(open_ms, 1), "generator_seconds": round(gen_s, 1), "first_request_wall_ms": round(first_wall_ms, 2),
            "walk_ms": round(walk_ms, 4), "select_ms": round(select_ms, 4), "offsets_ms": round(offsets_ms, 4), "device_ms": round(total_ms, 4),
            "request_wall_ms": [round(x, 3) for x in wall_ms], "nodes_per_s": nodes / (total_ms * 1e-3) if total_ms else 0.0,
            "kept_per_s": kept / (total_ms * 1e-3) if total_ms else 0.0, "rounds": int(rounds), "launches": int(launches),
            "scratch_bytes": int(scratch), "scratch_bytes_per_node": scratch / nodes if nodes else 0.0,
            "cpu_plain_walk_threads": cpu_threads, "cpu_plain_walk_ms": round(cpu_ms, 2), "cpu_plain_walk_steps": int(steps),
            "cpu_note": "lower bound on the reference's cost: its loop also calls sequence_len per step and is single-threaded",
            "parity_sample": len(picks), "parity_ok": bool(parity), "reference_paths_ok": bool(ids_ok),
            "source_fingerprint": bench.source_fingerprint(),
        }
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="small", choices=["tiny", "medium", "small", "full"])
    ap.add_argument("--interval", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--sample", type=int, default=4, help="paths of the parity check")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--out", default="", help="where the JSON line goes (default: profiles/r10_refpos_<size>.json)")
    a = ap.parse_args()
    res = run(a.size, a.interval, a.passes, a.sample, a.device, a.cpu_threads)
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", f"r10_refpos_{a.size}.json"), "w") as f:
        f.write(line + "\n")
    return 0 if res["parity_ok"] and res["reference_paths_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
