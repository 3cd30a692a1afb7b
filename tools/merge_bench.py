#!/usr/bin/env python3
"""GBWT merging on the device (include/gbwt_hip.h, "merging") on one GPU: two indexes over the paths of one bubble chain become one.

The chain of --sites x --haplotypes (2 alleles, mosaic, seed 42; default 100 000 x 1 000) is made by the host's sweep generator.  Its
paths are cut in two -- --shape halves: 500 + 500 haplotypes, insert: 990 + 10 (scaled to --haplotypes) --, each part is built with
GBWT.from_paths, and the two handles are merged --passes times by insertion and by MERGE_REBUILD.  The bytes of both results are compared
with the generator's own records at that full size.  One JSON line, also written to profiles/r16_merge_<shape>.json:

  insert: total_ms / decode_ms / walk_ms / interleave_ms / edges_ms / encode_ms   HIP events around the phases, median over the passes
          open_ms, metadata_ms, wall_ms          host clock: the open behind the merge, the metadata, the whole call
          walked_input, walked_sequences, walked_steps, walked_steps_per_s (over walk_ms)
          peak_scratch_bytes, scratch_bytes_per_visit (per visit of the result)
  rebuild: total_ms (edges + encode of the info are the last two phases only: wall_ms is the figure to compare), rounds, wall_ms
  rebuild_wall_over_insert_wall                  the ratio of the two medians, for the decision DESIGN.md 4j records"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def same_index(dev, s):
    data, starts = dev.records()
    return (bytes(data) == bytes(s.data()) and np.array_equal(starts, s.starts()) and
            (dev.sequences(), dev.len(), dev.alphabet_offset(), dev.alphabet_size()) == (s.sequences, s.size, s.alphabet_offset, s.alphabet_size))


def note(what, t0):
    print(f"[merge_bench] {what}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)


def timed_merges(G, a, b, algorithm, passes, s):
    infos, wall, parity = [], [], True
    for k in range(passes):
        t0 = time.perf_counter()
        merged = G.GBWT.merge(a, b, algorithm=algorithm)
        wall.append((time.perf_counter() - t0) * 1e3)
        infos.append(merged.last_merge_info())
        if k == passes - 1:
            parity = same_index(merged, s)
        merged.close()
    return infos, wall, parity


def run(shape="halves", sites=100000, haplotypes=1000, passes=3, device=0):
    import bench
    import gbwt_rs_amd as G
    from gbwt_rs_amd import synth as S
    t0 = time.perf_counter()
    s = S.Synth.chain(sites, haplotypes, alleles=2, model=S.MOSAIC, founders=32, switch_rate=2e-3, seed=42)
    note("host sweep generator", t0)
    paths = [s.path(h) for h in range(s.paths)]
    cut = haplotypes // 2 if shape == "halves" else haplotypes - max(1, haplotypes // 100)
    G.GBWT.merge(G.GBWT.from_paths([[2, 4, 6]], device=device), G.GBWT.from_paths([[2, 6]], device=device)).close()     # warm-up: the runtime, the kernels
    t0 = time.perf_counter()
    a, b = G.GBWT.from_paths(paths[:cut], device=device), G.GBWT.from_paths(paths[cut:], device=device)
    note("the two inputs built", t0)
    t0 = time.perf_counter()
    ins, ins_wall, ins_parity = timed_merges(G, a, b, G.MERGE_INSERT, passes, s)
    note(f"{passes} merges by insertion", t0)
    t0 = time.perf_counter()
    reb, reb_wall, reb_parity = timed_merges(G, a, b, G.MERGE_REBUILD, passes, s)
    note(f"{passes} merges by rebuild", t0)
    med = lambda infos, key: float(np.median([i[key] for i in infos]))
    phases = {k: med(ins, k) for k in ("decode_ms", "walk_ms", "interleave_ms", "edges_ms", "encode_ms")}
    total_ms = sum(phases.values())
    visits = int(ins[-1]["visits"])
    res = {
        "tool": "merge_bench", "shape": shape,
        "workload": f"bubble chain {sites} sites x {haplotypes} haplotypes (2 alleles, mosaic, seed 42), both orientations: paths 0 .. {cut - 1} + {cut} .. {haplotypes - 1}",
        "visits": visits, "sequences": int(ins[-1]["sequences"]), "records": int(ins[-1]["records"]), "data_bytes": int(ins[-1]["data_bytes"]),
        "insert": {"total_ms": total_ms, **phases, "open_ms": med(ins, "open_ms"), "metadata_ms": med(ins, "metadata_ms"), "wall_ms": float(np.median(ins_wall)),
                   "wall_ms_all": [round(x, 2) for x in ins_wall], "walked_input": int(ins[-1]["walked_input"]), "walked_sequences": int(ins[-1]["walked_sequences"]),
                   "walked_steps": int(ins[-1]["walked_steps"]),
                   "walked_steps_per_s": ins[-1]["walked_steps"] / (phases["walk_ms"] * 1e-3) if phases["walk_ms"] else 0.0,
                   "peak_scratch_bytes": int(ins[-1]["peak_scratch_bytes"]), "scratch_bytes_per_visit": ins[-1]["peak_scratch_bytes"] / visits if visits else 0.0,
                   "parity_ok": bool(ins_parity)},
        "rebuild": {"last_phases_ms": med(reb, "edges_ms") + med(reb, "encode_ms"), "rounds": int(reb[-1]["rounds"]), "open_ms": med(reb, "open_ms"),
                    "wall_ms": float(np.median(reb_wall)), "wall_ms_all": [round(x, 2) for x in reb_wall], "peak_scratch_bytes": int(reb[-1]["peak_scratch_bytes"]),
                    "parity_ok": bool(reb_parity)},
        "rebuild_wall_over_insert_wall": float(np.median(reb_wall)) / float(np.median(ins_wall)),
        "passes": passes, "source_fingerprint": bench.source_fingerprint(),
    }
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", choices=("halves", "insert"), default="halves")
    ap.add_argument("--sites", type=int, default=100000)
    ap.add_argument("--haplotypes", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="", help="where the JSON line goes (default: profiles/r16_merge_<shape>.json)")
    a = ap.parse_args()
    res = run(a.shape, a.sites, a.haplotypes, a.passes, a.device)
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", f"r16_merge_{a.shape}.json"), "w") as f:
        f.write(line + "\n")
    return 0 if res["insert"]["parity_ok"] and res["rebuild"]["parity_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
