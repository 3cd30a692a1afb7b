#!/usr/bin/env python3
"""GBWT path removal on the device (include/gbwt_hip.h, "removal") on one GPU: an index over the paths of one bubble chain loses some of them.

The chain of --sites x --haplotypes (2 alleles, mosaic, seed 42; default 100 000 x 1 000) is made by the host's sweep generator and built
with GBWT.from_paths.  --shape few removes every hundredth haplotype (10 of 1 000), half every second one (500), --passes times by
REMOVE_DELETE and by REMOVE_REBUILD, in turns.  The bytes of both results are compared with the host builder's records of the kept haplotypes
(Synth.from_paths: minutes at the full size, so --witness names a file the records are kept in, made on the first run and by
--witness-only, which needs no GPU).  One JSON line, also written to profiles/r17_remove_<shape>.json:

  delete: total_ms / decode_ms / walk_ms / compact_ms / edges_ms / encode_ms   HIP events around the phases, median over the passes
          open_ms, metadata_ms, wall_ms          host clock: the open behind the removal, the metadata, the whole call
          removed_sequences, removed_steps, removed_steps_per_s (over walk_ms)
          peak_scratch_bytes, scratch_bytes_per_position (per position, visit or sequence start, of the INPUT)
  rebuild: last_phases_ms (edges + encode of the info are the last two phases only: wall_ms is the figure to compare), rounds, wall_ms
  rebuild_wall_over_delete_wall                  the ratio of the two medians, for the decision DESIGN.md 4k records"""
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
    print(f"[remove_bench] {what}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)


def removed_haplotypes(shape, haplotypes):
    step = 100 if shape == "few" else 2
    return list(range(step - 1, haplotypes, step)) or [haplotypes - 1]


def chain_and_witness(shape, sites, haplotypes, witness):
    """(the chain, its paths, the removed path ids, the host builder's index of the kept paths)"""
    from gbwt_rs_amd import synth as S
    t0 = time.perf_counter()
    s = S.Synth.chain(sites, haplotypes, alleles=2, model=S.MOSAIC, founders=32, switch_rate=2e-3, seed=42)
    note("host sweep generator", t0)
    paths = [s.path(h) for h in range(s.paths)]
    removed = removed_haplotypes(shape, haplotypes)
    t0 = time.perf_counter()
    if witness and os.path.exists(witness):
        kept = S.Synth.from_file(witness)
        note("witness read", t0)
    else:
        gone = set(removed)
        kept = S.Synth.from_paths([p for h, p in enumerate(paths) if h not in gone])
        note("witness built on the host", t0)
        if witness:
            kept.save(witness)
    return s, paths, removed, kept


def timed_removals(G, x, removed, algorithms, passes, kept):
    """{algorithm: (infos, wall_ms, parity)}: the algorithms take turns, pass by pass, so that what else the machine does meets both"""
    runs = {a: ([], [], [True]) for a in algorithms}
    for _ in range(passes):
        for a in algorithms:
            infos, wall, parity = runs[a]
            t0 = time.perf_counter()
            out = x.remove_paths(removed, algorithm=a)
            wall.append((time.perf_counter() - t0) * 1e3)
            infos.append(out.last_remove_info())
            parity[0] = same_index(out, kept) and parity[0]     # every result, outside the clock
            out.close()
    return {a: (infos, wall, parity[0]) for a, (infos, wall, parity) in runs.items()}


def run(shape="few", sites=100000, haplotypes=1000, passes=3, device=0, witness=""):
    import bench
    import gbwt_rs_amd as G
    s, paths, removed, kept = chain_and_witness(shape, sites, haplotypes, witness)
    G.GBWT.from_paths([[2, 4, 6], [2, 6]], device=device).remove_paths([1], algorithm=G.REMOVE_DELETE).close()     # warm-up: the runtime, the kernels
    t0 = time.perf_counter()
    x = G.GBWT.from_paths(paths, device=device)
    note("the input built", t0)
    t0 = time.perf_counter()
    runs = timed_removals(G, x, removed, (G.REMOVE_DELETE, G.REMOVE_REBUILD), passes, kept)
    (dele, dele_wall, dele_parity), (reb, reb_wall, reb_parity) = runs[G.REMOVE_DELETE], runs[G.REMOVE_REBUILD]
    note(f"{passes} removals by deletion and {passes} by rebuild, in turns", t0)
    med = lambda infos, key: float(np.median([i[key] for i in infos]))
    phases = {k: med(dele, k) for k in ("decode_ms", "walk_ms", "compact_ms", "edges_ms", "encode_ms")}
    positions = int(x.len())
    res = {
        "tool": "remove_bench", "shape": shape,
        "workload": f"bubble chain {sites} sites x {haplotypes} haplotypes (2 alleles, mosaic, seed 42), both orientations: {len(removed)} haplotypes removed "
                    f"({removed[0]}, {removed[1] if len(removed) > 1 else removed[0]}, ...)",
        "input_positions": positions, "visits": int(dele[-1]["visits"]), "sequences": int(dele[-1]["sequences"]), "records": int(dele[-1]["records"]),
        "data_bytes": int(dele[-1]["data_bytes"]),
        "delete": {"total_ms": sum(phases.values()), **phases, "open_ms": med(dele, "open_ms"), "metadata_ms": med(dele, "metadata_ms"), "wall_ms": float(np.median(dele_wall)),
                   "wall_ms_all": [round(w, 2) for w in dele_wall], "removed_sequences": int(dele[-1]["removed_sequences"]), "removed_steps": int(dele[-1]["removed_steps"]),
                   "removed_steps_per_s": dele[-1]["removed_steps"] / (phases["walk_ms"] * 1e-3) if phases["walk_ms"] else 0.0,
                   "peak_scratch_bytes": int(dele[-1]["peak_scratch_bytes"]), "scratch_bytes_per_position": dele[-1]["peak_scratch_bytes"] / positions if positions else 0.0,
                   "parity_ok": bool(dele_parity)},
        "rebuild": {"last_phases_ms": med(reb, "edges_ms") + med(reb, "encode_ms"), "rounds": int(reb[-1]["rounds"]), "open_ms": med(reb, "open_ms"),
                    "wall_ms": float(np.median(reb_wall)), "wall_ms_all": [round(w, 2) for w in reb_wall], "peak_scratch_bytes": int(reb[-1]["peak_scratch_bytes"]),
                    "parity_ok": bool(reb_parity)},
        "rebuild_wall_over_delete_wall": float(np.median(reb_wall)) / float(np.median(dele_wall)),
        "passes": passes, "source_fingerprint": bench.source_fingerprint(),
    }
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", choices=("few", "half"), default="few")
    ap.add_argument("--sites", type=int, default=100000)
    ap.add_argument("--haplotypes", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--witness", default="", help="a .gbwt file that keeps the host builder's index of the kept haplotypes between runs")
    ap.add_argument("--witness-only", action="store_true", help="make the --witness file and stop (no GPU)")
    ap.add_argument("--out", default="", help="where the JSON line goes (default: profiles/r17_remove_<shape>.json)")
    a = ap.parse_args()
    if a.witness_only:
        if not a.witness:
            ap.error("--witness-only needs --witness")
        chain_and_witness(a.shape, a.sites, a.haplotypes, a.witness)
        return 0
    res = run(a.shape, a.sites, a.haplotypes, a.passes, a.device, a.witness)
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", f"r17_remove_{a.shape}.json"), "w") as f:
        f.write(line + "\n")
    return 0 if res["delete"]["parity_ok"] and res["rebuild"]["parity_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
