#!/usr/bin/env python3
"""Locate queries (include/gbwt_hip.h, "locate") on BASELINE config 3's index (tools/configs.py: search) on one GPU.

The bubble chain of config 3 at --size (full: 1.1 M sites x 5 008 haplotypes; small: a tenth of the sites and of the haplotypes), the million
10-node queries built as src/bin/benchmark.rs:124-153 builds them, searched on the device; their final states, still in HBM, are located
(gbwt_hip_search_device -> gbwt_hip_locate_states_device).  One JSON line, also written to profiles/r12_locate_<size>.json:

  build_ms / build_launches     the locate index, built by the first request (HIP events around the build)
  index_bytes                   what it adds to the handle's device bytes; sampled_records / table_positions / end_entries: its shape
  positions                     BWT positions behind the final states (the rows of a plain request together)
  plain / unique                median over --passes requests behind --warmup unmeasured ones: walk_ms (k_locate), sort_ms (sort, flags, scan,
                                compaction), positions_per_s = positions / (walk_ms + sort_ms), wall_ms of the whole call
  steps_per_position            LF steps per located position, counted by a launch of its own with a counter (never the timed one)
  parity                        a seeded sample of the located positions against the oracle: GBWT::backward to the start of the sequence

No speed-up is stated: the reference has no locate to compare with."""
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

SIZES = {
    "small": {"sites": 110000, "haplotypes": 500, "n_queries": 1000000},
    "full": {"sites": 1100000, "haplotypes": 5008, "n_queries": 1000000},
}


def owner_by_walking_back(oracle, starts, pos):
    """The sequence whose visit `pos` is: GBWT::backward (src/gbwt.rs:236-250) until the sequence starts."""
    while True:
        before = oracle.backward(pos)
        if before is None:
            return starts[pos]
        pos = before


def run(size="small", passes=5, warmup=2, sample=12, device=0, length=10):
    import torch
    import bench
    import configs as K
    import gbwt_rs_amd as G
    import oracle_lib as O
    from gbwt_rs_amd import synth as S
    p = SIZES[size]
    t0 = time.perf_counter()
    s = S.Synth.chain(p["sites"], p["haplotypes"], alleles=2, model=S.MOSAIC, founders=32, switch_rate=2e-3, seed=42)
    gen_s = time.perf_counter() - t0
    dev = G.GBWT.from_records(s.data(), s.starts(), s.alphabet_offset, s.alphabet_size, s.sequences, s.size, True, device=device)
    queries = K.make_benchmark_queries(dev, s.alphabet_offset + 1, s.alphabet_size, p["n_queries"], length, 7)
    n = queries.shape[0]
    d_q = torch.from_numpy(queries.view(np.int64)).cuda(device)
    searched = dev.search_device(d_q.data_ptr(), n, length)
    mem0 = dev.memory_usage()
    t0 = time.perf_counter()
    rows = dev.locate_states_device(searched, False)       # (the first request builds the index)
    first_wall_ms = (time.perf_counter() - t0) * 1e3
    info = dev.locate_index_info()
    positions = int(rows.total)
    modes = {}
    for name, unique in (("plain", False), ("unique", True)):
        for _ in range(warmup):
            dev.locate_states_device(searched, unique)
        walk, sort, wall, total = [], [], [], 0
        for _ in range(passes):
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            out = dev.locate_states_device(searched, unique)
            wall.append((time.perf_counter() - t0) * 1e3)
            w, q = dev.last_locate_ms()
            walk.append(w), sort.append(q)
            total = int(out.total)
        device_ms = float(np.median(walk)) + float(np.median(sort))
        modes[name] = {"walk_ms": float(np.median(walk)), "sort_ms": float(np.median(sort)), "wall_ms": float(np.median(wall)), "ids": total,
                       "positions_per_s": positions / (device_ms * 1e-3) if device_ms else 0.0,
                       "walk_ms_all": [round(x, 4) for x in walk], "sort_ms_all": [round(x, 4) for x in sort]}
    mem1 = dev.memory_usage()
    states, found = dev.states_to_host(searched)
    steps, counted = dev.locate_count_steps(states)
    # parity on a seeded sample of the positions
    oracle = O.OracleGBWT.from_bwt(O.OracleBWT.from_parts(s.data(), s.starts()), s.sequences, s.size, s.alphabet_offset, s.alphabet_size, True)
    starts = {oracle.start(k): k for k in range(oracle.sequences())}
    rng = np.random.default_rng(11)
    picks = rng.choice(n, size=min(sample, n), replace=False)
    parity = bool(found.all()) and counted == positions
    for k in picks.tolist():
        st = states[k]
        offset = int(st["start"]) + int(rng.integers(0, int(st["end"]) - int(st["start"])))
        ids, valid = dev.locate_positions(np.array([[int(st["node"]), offset]], dtype=np.uint64))
        parity &= bool(valid[0]) and int(ids[0]) == owner_by_walking_back(oracle, starts, (int(st["node"]), offset))
    del d_q
    res = {
        "tool": "locate_bench", "size": size,
        "workload": f"BASELINE config 3 shape: bubble chain {p['sites']} sites x {p['haplotypes']} haplotypes (mosaic, seed 42), the final states of {n} queries of {length} nodes (seed 7)",
        "queries": int(n), "positions": positions, "positions_per_state": positions / n if n else 0.0, "generator_seconds": round(gen_s, 1),
        "build_ms": info["build_ms"], "build_launches": info["build_launches"], "first_request_wall_ms": round(first_wall_ms, 2),
        "interval": info["interval"], "index_bytes": info["device_bytes"], "sampled_records": info["sampled_records"], "table_positions": info["table_positions"],
        "end_entries": info["end_entries"], "index_device_bytes_before": mem0["index_device_bytes"], "index_device_bytes_after": mem1["index_device_bytes"],
        "workspace_device_bytes": mem1["workspace_device_bytes"],
        "plain": modes["plain"], "unique": modes["unique"], "lf_steps": int(steps), "steps_per_position": steps / positions if positions else 0.0,
        "passes": passes, "warmup": warmup, "parity_sample": int(len(picks)), "parity_ok": bool(parity),
        "source_fingerprint": bench.source_fingerprint(),
    }
    dev.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="small", choices=sorted(SIZES))
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=12, help="positions of the parity check")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="", help="where the JSON line goes (default: profiles/r12_locate_<size>.json)")
    a = ap.parse_args()
    res = run(a.size, a.passes, a.warmup, a.sample, a.device)
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", f"r12_locate_{a.size}.json"), "w") as f:
        f.write(line + "\n")
    return 0 if res["parity_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
